#!/usr/bin/env python
"""Environment-steps per second of batched worlds (rbhip.BatchWorld) against
one World stepping the same scene.

The scene is the reference's multi_sphere4 (models/multi_sphere.xml: four
balls) in f64.  A batch of E environments runs a restitution sweep
(sim_overrides.py's knob, 0.5 .. 1.0 over the environments); every timed
window is `--steps` steps around one synchronous step call, after a warm-up
of the same length, from the same start state, repeated `--reps` times so the
spread is visible.  In the same run one World(multi_sphere4) steps `--steps`
steps the same number of times: without batches that is the only way to run
the scene, one World call per environment.

Prints one JSON line and writes it to --out (default
profiles/batch/batch_bench.json).  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rigidbody-simulation_amd"))


def _summary(rates):
    r = sorted(rates)
    return dict(median=r[len(r) // 2], min=r[0], max=r[-1], reps=rates)


def bench_batch(rb, sc, E, steps, reps, dtype):
    q = np.broadcast_to(sc.qpos0, (E, sc.n, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (E, sc.n, 6)).copy()
    with rb.BatchWorld(sc, E, dtype=dtype) as b:
        b.set_params(restitution=np.linspace(0.5, 1.0, E))
        b.step(steps)                                   # warm-up
        rates = []
        for _ in range(reps):
            b.set_state(q, v)
            t0 = time.perf_counter()
            failed = b.step(steps)                      # synchronous
            dt = time.perf_counter() - t0
            if failed:
                raise RuntimeError(f"{failed} environments failed")
            rates.append(E * steps / dt)
    return _summary(rates)


def bench_world(rb, sc, steps, reps, dtype):
    with rb.World(sc, dtype=dtype) as w:
        w.step(steps)                                   # warm-up (captures the step graph)
        rates = []
        for _ in range(reps):
            w.set_state(sc.qpos0, sc.qvel0)
            t0 = time.perf_counter()
            w.step(steps)                               # synchronous
            rates.append(steps / (time.perf_counter() - t0))
    return _summary(rates)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="+", default=[1, 1024, 16384, 262144])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "batch_bench.json"))
    a = ap.parse_args()

    import rbhip
    from rbhip import scenes
    rbhip.load()
    sc = scenes.multi_sphere4()
    res = dict(bench="batch_bench", scene="multi_sphere4", bodies_per_env=sc.n, dtype=a.dtype, steps=a.steps,
               unit="environment-steps per second", version=rbhip.load().rb_version().decode())
    res["world"] = bench_world(rbhip, sc, a.steps, a.reps, a.dtype)
    res["batch"] = {str(E): bench_batch(rbhip, sc, E, a.steps, a.reps, a.dtype) for E in a.envs}
    res["world_after"] = bench_world(rbhip, sc, a.steps, a.reps, a.dtype)
    w = res["world"]["median"]
    res["ratio_vs_world"] = {E: dict(median=r["median"] / w, min=r["min"] / w, max=r["max"] / w)
                             for E, r in res["batch"].items()}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
