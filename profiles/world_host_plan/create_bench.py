#!/usr/bin/env python
"""create_bench.py [--package DIR] [--creations 20]: the time to create a world
of 65,536 spheres (the flat scene C3) and take its first step, per creation:
rb_world_create with its plan and allocations, the constants' and the state's
upload, the table's prime and one synchronous step, then the world's teardown
(outside the timed window).  One warm-up creation first (HIP's context, the
library's load), then `--creations` timed ones.  Prints one JSON line: the
process's median in seconds, and every value.

--package DIR: the directory that holds the `rbhip` package to time (default:
this tree's), so that one script times both sides of an A/B."""
import argparse, json, os, statistics, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--package", default=os.path.join(ROOT, "rigidbody-simulation_amd"))
ap.add_argument("--creations", type=int, default=20)
a = ap.parse_args()
sys.path.insert(0, a.package)
import rbhip
from rbhip import scenes

sc = scenes.flat_spheres(256, 256, seed=0)


def once():
    t0 = time.perf_counter()
    w = rbhip.World(sc, device=0)
    w.step(1)
    t = time.perf_counter() - t0
    w.close()
    return t


once()
ts = [once() for _ in range(a.creations)]
print(json.dumps(dict(metric="world create + first step", unit="s", bodies=sc.n, creations=a.creations,
                      median=statistics.median(ts), min=min(ts), max=max(ts), values=ts)))
