"""Diagnostic: one 8,192-body shard of C3 (8 in-process shards on one GPU,
host-driven exchange as in scripts/shard_step_run.py): the step kernel's
HIP-event time per launch on rank 0 over 100 steps after 50, the parent's
library (gpu_jobs/parent/librbhip.so, built from the parent commit, kept out
of git) and this tree's interleaved in one process, five rounds.  Not part of
the product.  The tail of profiles/lead_block/shapes_ab.log is its output."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rigidbody-simulation_amd"))
import torch
torch.cuda.init()
from rbhip import _lib, scenes
import rbhip.world as W
from rbhip.shard import wrap_gpos
libs = [("parent", os.path.join(ROOT, "gpu_jobs/parent/librbhip.so")),
        ("child", os.path.join(ROOT, "rigidbody-simulation_amd/rbhip/librbhip.so"))]
sc = scenes.make("c3")
P, WARM, K = 8, 50, 100
res = {}
for rnd in range(5):
    for name, lib in libs:
        _lib._lib = None
        _lib.load(lib)
        worlds = [W.World(sc, rank=r, world_size=P) for r in range(P)]
        for t in range(WARM + K):
            if t == WARM:
                worlds[0].kernel_timing(True)
            for w in worlds:
                w.shard_step()
            for w in worlds:
                w.sync()
            bufs = [wrap_gpos(w, torch) for w in worlds]
            n = bufs[0][1]
            for r, (buf, _) in enumerate(bufs):
                for o, (obuf, _) in enumerate(bufs):
                    if o != r:
                        buf[o * n:(o + 1) * n].copy_(obuf[o * n:(o + 1) * n])
            torch.cuda.synchronize()
            for w in worlds:
                w.shard_exchange_done()
        avg, cnt = worlds[0].kernel_timing(False)
        form = worlds[0].stats()["form"]
        for w in worlds:
            w.close()
        res.setdefault(name, []).append(avg * 1e3)
        print(f"round {rnd} c3 shard 1/8 ({sc.n // P} bodies) {name:7s} {avg * 1e3:8.3f} us/launch over {cnt} launches, form {form}", flush=True)
for name, t in res.items():
    print(f"SUMMARY c3 shard 1/8 {name:7s} min {min(t):8.3f} max {max(t):8.3f} median {sorted(t)[len(t) // 2]:8.3f} us/launch  all {' '.join(f'{x:.3f}' for x in t)}")
