#!/usr/bin/env python
"""What a closed loop around a World costs per iteration, through device
tensors and through host arrays, in one process.

An iteration: read the state, compute the applied forces F = -k v from it
(a drag on the linear velocity; no torque: with k = 0.5 and dt = 0.01 an
explicit drag -k w on a sphere of inertia 8.4e-4 would grow the spin five-fold
per step), set them, take one step.

  device   get_state_device, F in torch, set_xfrc_device, step_async(1) on
           torch's current stream, no synchronisation inside the loop; the
           clock runs over `--iters` iterations between two synchronisations
  host     get_state, F in numpy, set_xfrc, step(1): every call waits
  steps    step_async(1) alone, `--iters` of them between two synchronisations
           (the step's share of the device loop; forces stay set)

Each after a warm-up of `--warmup` iterations from the scene's start state,
repeated `--reps` times; microseconds per iteration, median and min / max of
the repeats.  Scenes: C3 (65,536 spheres, the scene bench.py measures) and
flat_spheres(64, 64).  Prints one JSON line per scene and, with --out DIR,
writes them to DIR/<scene>.json.  Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rigidbody-simulation_amd"))

K = 0.5


def _summary(x):
    r = sorted(x)
    return dict(median=r[len(r) // 2], min=r[0], max=r[-1], reps=x)


def measure(name, sc, a):
    import numpy as np
    import torch
    import rbhip
    out = {"scene": name, "bodies": sc.n, "dtype": a.dtype, "iters": a.iters, "warmup": a.warmup, "k": K,
           "unit": "microseconds per iteration (host clock between two synchronisations)"}
    with rbhip.World(sc, dtype=a.dtype) as w:
        w.set_stream(torch.cuda.current_stream().cuda_stream)
        dev = f"cuda:{w.device}"
        q = torch.empty((sc.n, 7), dtype=torch.float64, device=dev)
        v = torch.empty((sc.n, 6), dtype=torch.float64, device=dev)
        f = torch.zeros((sc.n, 6), dtype=torch.float64, device=dev)

        def device_loop(n):
            for _ in range(n):
                w.get_state_device(q, v)
                torch.mul(v[:, :3], -K, out=f[:, :3])
                w.set_xfrc_device(f)
                w.step_async(1)

        def steps_only(n):
            for _ in range(n):
                w.step_async(1)

        def host_loop(n):
            for _ in range(n):
                _, hv = w.get_state()
                hf = np.zeros((sc.n, 6))
                hf[:, :3] = -K * hv[:, :3]
                w.set_xfrc(hf)
                w.step(1)

        def timed(loop):
            reps = []
            for _ in range(a.reps):
                w.set_xfrc(None)
                w.set_state(sc.qpos0, sc.qvel0)
                loop(a.warmup)
                w.sync()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loop(a.iters)
                w.sync()
                torch.cuda.synchronize()
                reps.append((time.perf_counter() - t0) / a.iters * 1e6)
            return _summary(reps)

        out["device_loop_us"] = timed(device_loop)
        dq, dv = w.get_state()
        out["steps_only_us"] = timed(lambda n: (w.set_xfrc_device(f), steps_only(n)))
        out["host_loop_us"] = timed(host_loop)
        hq, hv = w.get_state()
        # both loops took the same steps from the same state with the same arithmetic
        out["loops_agree_in_bits"] = bool(np.array_equal(dq.view(np.uint64), hq.view(np.uint64))
                                          and np.array_equal(dv.view(np.uint64), hv.view(np.uint64)))
        out["form"] = w.stats()["form"]
    out["host_over_device"] = out["host_loop_us"]["median"] / out["device_loop_us"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--out", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.iters < 200:
        ap.error("--iters: at least 200 (a shorter window measures the clock)")

    import rbhip
    from rbhip import scenes
    rbhip.load()
    for name, sc in (("c3", scenes.make("c3")), ("flat_spheres_64_64", scenes.flat_spheres(64, 64))):
        line = measure(name, sc, a)
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, name + ".json"), "w") as fh:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
