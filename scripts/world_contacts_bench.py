#!/usr/bin/env python
"""What the contact list of a World's current state costs, by each route, in
one process.

Per scene, after `--settle` steps from the scene's start state:

  (a) step          step_async(1), `--iters` of them between two synchronisations
  (b) recorded      the only route before the query: record_contacts(True),
                    step(1), contacts() (a step, recording traffic, a CSR
                    download; partner, kind and dist only) -- host clock per call
  (c) query         query_contacts(max_records=R): the host form, host clock per call
  (d) query_device  query_contacts_device(out=...) on torch's current stream,
                    device events around `--iters` calls; split into the fill of
                    the query's table (events around a one-body counts-only call:
                    the generation and error words, the insert of every body and a
                    one-wave query kernel) and the rest, the query kernel

for R = max_records in (8, 0).  (b) changes the state, so each repeat starts
from the settled state again; (c) and (d) change nothing.  Microseconds,
median and min / max of `--reps` repeats.  (d)'s written bytes, count * (4 + R
* (8 + 7 * elem)), are reported beside its kernel time as a fraction of the
HBM peak (8.0 TB/s, MI355X): the lists are small, so this says how far from a
bandwidth bound the query is, not how well it uses the memory.

Scenes: C3 (65,536 spheres, the scene bench.py measures) after 500 steps, and
box_pile(8, 8, 3).  Prints one JSON line and writes it to
profiles/world_contacts/world_contacts_bench.json (--out).  Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rigidbody-simulation_amd"))

HBM_PEAK = 8.0e12      # bytes per second


def _summary(x):
    r = sorted(x)
    return dict(median=r[len(r) // 2], min=r[0], max=r[-1], reps=x)


def measure(name, sc, settle, max_partners, a):
    import torch
    import rbhip
    elem = 8 if a.dtype == "f64" else 4
    out = {"scene": name, "bodies": sc.n, "dtype": a.dtype, "settle_steps": settle, "iters": a.iters, "reps": a.reps,
           "unit": "microseconds per call"}
    with rbhip.World(sc, dtype=a.dtype, max_partners=max_partners) as w:
        w.set_stream(torch.cuda.current_stream().cuda_stream)
        w.step(settle)
        q0, v0 = w.get_state()
        out["form"] = w.stats()["form"]

        def host_clock(call, n, reset=False):
            reps = []
            for _ in range(a.reps):
                if reset:
                    w.set_state(q0, v0)
                call()                                   # warm-up of this shape
                if reset:
                    w.set_state(q0, v0)
                w.sync()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    call()
                w.sync()
                torch.cuda.synchronize()
                reps.append((time.perf_counter() - t0) / n * 1e6)
            return _summary(reps)

        def events(call, n):
            reps = []
            for _ in range(a.reps):
                call()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    call()
                e1.record()
                torch.cuda.synchronize()
                reps.append(e0.elapsed_time(e1) / n * 1e3)
            return _summary(reps)

        # (a) a step (the state moves on; put back afterwards)
        out["step_us"] = host_clock(lambda: w.step_async(1), a.iters)
        w.set_state(q0, v0)
        # (b) the recorded route: a few steps per repeat from the settled state
        w.record_contacts(True)

        def recorded():
            w.step(1)
            return w.contacts()
        out["recorded_us"] = host_clock(recorded, a.host_iters, reset=True)
        out["recorded_contacts"] = int(recorded()[0].sum())
        w.record_contacts(False)
        w.set_state(q0, v0)
        w.sync()
        one = w.query_contacts_device(first=0, count=1, max_records=0)
        out["fill_us"] = events(lambda: w.query_contacts_device(first=0, count=1, out=one), a.iters)
        for R in (8, 0):
            r = {}
            r["query_us"] = host_clock(lambda: w.query_contacts(max_records=R), a.host_iters)
            con = w.query_contacts(max_records=R)
            r["contacts"], r["truncated_bodies"] = int(con.counts.sum()), int(con.truncated)
            dev = w.query_contacts_device(max_records=R)
            r["query_device_us"] = events(lambda: w.query_contacts_device(out=dev), a.iters)
            kern = max(r["query_device_us"]["median"] - out["fill_us"]["median"], 1e-3)
            r["query_kernel_us"] = kern
            r["written_bytes"] = sc.n * (4 + R * (8 + 7 * elem))
            r["written_over_hbm_peak_of_kernel"] = r["written_bytes"] / (kern * 1e-6) / HBM_PEAK
            r["written_over_hbm_peak_of_call"] = r["written_bytes"] / (r["query_device_us"]["median"] * 1e-6) / HBM_PEAK
            r["device_over_recorded"] = r["query_device_us"]["median"] / out["recorded_us"]["median"]
            r["device_over_step"] = r["query_device_us"]["median"] / out["step_us"]["median"]
            r["host_over_recorded"] = r["query_us"]["median"] / out["recorded_us"]["median"]
            out[f"R{R}"] = r
        # the queries left the state where it was
        import numpy as np
        q1, v1 = w.get_state()
        out["state_unchanged"] = bool(np.array_equal(q0.view(np.uint64), q1.view(np.uint64))
                                      and np.array_equal(v0.view(np.uint64), v1.view(np.uint64)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=200, help="calls per timed window of the enqueued routes")
    ap.add_argument("--host-iters", type=int, default=20, help="calls per timed window of the synchronous routes")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--settle", type=int, default=500, help="steps before the C3 measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_contacts"), metavar="DIR")
    a = ap.parse_args()

    import rbhip
    from rbhip import scenes
    rbhip.load()
    line = {"script": "scripts/world_contacts_bench.py", "hbm_peak_bytes_per_s": HBM_PEAK, "scenes": []}
    for name, sc, settle, maxp in (("c3", scenes.make("c3"), a.settle, 16), ("box_pile_8_8_3", scenes.box_pile(8, 8, 3), 200, 32)):
        line["scenes"].append(measure(name, sc, settle, maxp, a))
    print(json.dumps(line), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "world_contacts_bench.json"), "w") as fh:
        fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
