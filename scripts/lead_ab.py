"""Diagnostic: A/B of library builds ("lead block") — per-step device
time of K graph-replayed steps after W warm steps, as scripts/help_search_ab.py
measures it, interleaved in one process over the builds, five rounds; unlike
that script it forces no form: every world steps as the product would.  Not
part of the product.

    python scripts/lead_ab.py LABEL=PATH,LABEL=PATH,... CONFIG:WARM:K,...

e.g. parent=gpu_jobs/parent/librbhip.so,new=rigidbody-simulation_amd/rbhip/librbhip.so
     c3:45:20,c3:450:400,c4:450:400,c5:450:400,flat32k:450:400,c2:450:400
(paths relative to the repository; the parent's library built from the parent
commit into a directory kept out of git).  profiles/lead_block/shapes_ab.log
and variants_ab.log are its output."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rigidbody-simulation_amd"))
import torch
torch.cuda.init()
from rbhip import _lib, scenes
import rbhip.world as W
variants = [tuple(v.split("=", 1)) for v in sys.argv[1].split(",")]
shapes = [(c, int(w), int(k)) for c, w, k in (s.split(":") for s in sys.argv[2].split(","))]
scs = {c: (scenes.flat_spheres(256, 128) if c == "flat32k" else scenes.make(c)) for c, _, _ in shapes}
res = {}
for rnd in range(5):
    for name, lib in variants:
        _lib._lib = None
        _lib.load(os.path.join(ROOT, lib))
        for cfg, warm, K in shapes:
            kw = {"max_partners": 32} if cfg == "c4" else {}
            with W.World(scs[cfg], **kw) as w:
                w.set_stream(torch.cuda.current_stream().cuda_stream)
                w.step(warm - K)
                w.step(K)
                w.sync()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                w.step_async(K)
                e1.record()
                w.sync()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / K
                st = w.stats()
            res.setdefault((cfg, warm, K, name), []).append(us)
            print(f"round {rnd} {cfg} steps {warm + 1}-{warm + K} {name:9s} {us:8.3f} us/step form {st.get('hashed_form')} "
                  f"maxp {st.get('max_partners')} share {st.get('help_search')}", flush=True)
for (cfg, warm, K, name), t in res.items():
    print(f"SUMMARY {cfg} steps {warm + 1}-{warm + K} {name:9s} min {min(t):8.3f} max {max(t):8.3f} "
          f"median {sorted(t)[len(t) // 2]:8.3f} us/step  all {' '.join(f'{x:.3f}' for x in t)}")
