#!/usr/bin/env python
"""What the impulse query of a World's current state costs beside the contact
query and a step, in one process.

Per scene, after `--settle` steps from the scene's start state, each call timed
in windows of `--iters` (20) calls closed by one sync(), `--reps` (7) windows
after a warm-up of the same shape; host clock, microseconds per call, median
and min / max of the windows:

  impulses_device   query_impulses_device(out=...) at R = max_records in (0, 8)
  contacts_device   query_contacts_device(out=..., geometry=False) at the same R
  step              step_async(1) (the state moves on; it is put back afterwards)

Both queries fill the query's table first (one insert of every body per call);
the impulse query then runs the contact query's search and walk plus the solve.
The queries change nothing, which is checked at the end.

Scenes: C3 (65,536 spheres, the scene bench.py measures) after 500 steps, and
box_pile(8, 8, 3) after 200.  Prints one JSON line and writes it to
profiles/world_impulses/world_impulses_bench.json (--out, --name).  Needs the
GPU.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rigidbody-simulation_amd"))


def _summary(x):
    r = sorted(x)
    return dict(median=r[len(r) // 2], min=r[0], max=r[-1], reps=x)


def measure(name, sc, settle, max_partners, a):
    import numpy as np
    import torch
    import rbhip
    out = {"scene": name, "bodies": sc.n, "dtype": a.dtype, "settle_steps": settle, "iters": a.iters, "reps": a.reps,
           "unit": "microseconds per call"}
    with rbhip.World(sc, dtype=a.dtype, max_partners=max_partners) as w:
        w.set_stream(torch.cuda.current_stream().cuda_stream)
        w.step(settle)
        q0, v0 = w.get_state()
        out["form"] = w.stats()["form"]

        def windows(call):
            reps = []
            call()                                       # warm-up of this shape
            w.sync()
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    call()
                w.sync()
                reps.append((time.perf_counter() - t0) / a.iters * 1e6)
            return _summary(reps)

        for R in (0, 8):
            r = {}
            imp = w.query_impulses_device(max_records=R)
            con = w.query_contacts_device(max_records=R, geometry=False)
            w.sync()
            r["contacts"] = int(con.counts.clamp(min=0).sum().item())
            r["bodies_past_R"] = int((con.counts > R).sum().item())
            r["applied"] = int((imp.net != 0).any(dim=-1).sum().item())      # bodies with a net contact impulse
            r["impulses_device_us"] = windows(lambda: w.query_impulses_device(out=imp))
            r["contacts_device_us"] = windows(lambda: w.query_contacts_device(out=con, geometry=False))
            r["impulses_over_contacts"] = r["impulses_device_us"]["median"] / r["contacts_device_us"]["median"]
            out[f"R{R}"] = r
        q1, v1 = w.get_state()
        out["state_unchanged"] = bool(np.array_equal(q0.view(np.uint64), q1.view(np.uint64))
                                      and np.array_equal(v0.view(np.uint64), v1.view(np.uint64)))
        out["step_us"] = windows(lambda: w.step_async(1))
        w.set_state(q0, v0)
        for R in (0, 8):
            out[f"R{R}"]["impulses_over_step"] = out[f"R{R}"]["impulses_device_us"]["median"] / out["step_us"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
    ap.add_argument("--reps", type=int, default=7, help="timed windows per call")
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--settle", type=int, default=500, help="steps before the C3 measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_impulses"), metavar="DIR")
    ap.add_argument("--name", default="world_impulses_bench", help="the JSON file's name, without .json")
    a = ap.parse_args()

    import rbhip
    from rbhip import scenes
    rbhip.load()
    line = {"script": "scripts/world_impulses_bench.py", "scenes": []}
    for name, sc, settle, maxp in (("c3", scenes.make("c3"), a.settle, 16), ("box_pile_8_8_3", scenes.box_pile(8, 8, 3), 200, 32)):
        line["scenes"].append(measure(name, sc, settle, maxp, a))
    print(json.dumps(line), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name + ".json"), "w") as fh:
        fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
