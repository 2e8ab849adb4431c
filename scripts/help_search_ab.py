"""Diagnostic: A/B of the wide + helper form's shared search —
per-step device time of K graph-replayed steps after W warm steps, as
scripts/epoch_ab.py measures it, interleaved in one process over library
builds and RBHIP_HELP_SEARCH settings.  Not part of the product.

    python scripts/help_search_ab.py [--parent PATH] [--rounds 5]
        [--shapes c3:45:20,c3:450:400,c4:450:400,c5:450:400,flat32k:450:400,c2:450:400]
        [--variants LABEL=PATH,...]

Without --variants: the parent library (if given), this tree's library with
the shared search on ("child") and off ("child_off").  With --variants: the
parent library (if given), this tree's library and the listed builds (e.g.
made with WEXTRA=-DRB_SHARE_QBATCH=6 or -DRB_SHARE_SPLIT=5 and OUT=PATH), all
with the shared search on.  flat32k is flat_spheres(256, 128).
profiles/help_search/shapes_ab.log and variants_ab.log are its output (the
parent's library there was built from the parent commit into
gpu_jobs/parent/librbhip.so, a directory kept out of git).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rigidbody-simulation_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "rigidbody-simulation_amd", "rbhip", "librbhip.so"))
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variants", default="")
    ap.add_argument("--shapes", default="c3:45:20,c3:450:400,c4:450:400,c5:450:400,flat32k:450:400,c2:450:400")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from rbhip import _lib, scenes
    import rbhip.world as W

    shapes = [(c, int(w), int(k)) for c, w, k in (s.split(":") for s in a.shapes.split(","))]
    scs = {c: (scenes.flat_spheres(256, 128) if c == "flat32k" else scenes.make(c)) for c, _, _ in shapes}
    if a.variants:
        variants = (([("parent", a.parent, None)] if a.parent else []) + [("child", a.lib, "1")] +
                    [tuple(v.split("=", 1)) + ("1",) for v in a.variants.split(",") if v])
    else:
        variants = ([("parent", a.parent, None)] if a.parent else []) + [("child", a.lib, "1"), ("child_off", a.lib, "0")]
    res = {}
    for rnd in range(a.rounds):
        for name, lib, share in variants:
            _lib._lib = None
            _lib.load(lib)
            os.environ.pop("RBHIP_HELP_SEARCH", None)
            if share is not None:
                os.environ["RBHIP_HELP_SEARCH"] = share
            for cfg, warm, K in shapes:
                kw = {"max_partners": 32} if cfg == "c4" else {}
                with W.World(scs[cfg], **kw) as w:
                    w.set_stream(torch.cuda.current_stream().cuda_stream)
                    w.step(warm - K)
                    w.step(K)                    # captures the K-step graph the window replays
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


if __name__ == "__main__":
    main()
