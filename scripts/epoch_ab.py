"""Diagnostic: A/B of RBHIP_TABLE_EPOCH settings (and of a second library
build, e.g. the parent commit's) on bench.py's windows, interleaved in one
process: per-step device time of K graph-replayed steps after W warm steps,
as scripts/window_time.py measures it.  Not part of the product.

    python scripts/epoch_ab.py [--parent PATH] [--epochs 1,2,4,8,16] [--rounds 5]
                               [--shapes c3:450:400,c3:45:20,c4:450:400,c2:450:400]
                               [--variants LABEL=PATH@EPOCH,...]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rigidbody-simulation_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "rigidbody-simulation_amd", "rbhip", "librbhip.so"))
    ap.add_argument("--parent", default=None, help="a second library, timed as variant 'parent'")
    ap.add_argument("--epochs", default="1,2,4,8,16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variants", default="", help="further library builds: LABEL=PATH@EPOCH,...")
    ap.add_argument("--shapes", default="c3:450:400,c3:45:20,c4:450:400,c2:450:400")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from rbhip import _lib, scenes
    import rbhip.world as W

    shapes = [(c, int(w), int(k)) for c, w, k in (s.split(":") for s in a.shapes.split(","))]
    scs = {c: scenes.make(c) for c, _, _ in shapes}
    variants = ([("parent", a.parent, None)] if a.parent else []) + [(f"E={e}", a.lib, e) for e in a.epochs.split(",") if e]
    # further builds: LABEL=PATH@EPOCH,...
    for v in a.variants.split(","):
        if v:
            label, rest = v.split("=", 1)
            path, e = rest.rsplit("@", 1)
            variants.append((label, path, e))
    res = {}
    for rnd in range(a.rounds):
        for name, lib, e in variants:
            _lib._lib = None
            _lib.load(lib)
            if e is None:
                os.environ.pop("RBHIP_TABLE_EPOCH", None)
            else:
                os.environ["RBHIP_TABLE_EPOCH"] = e
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
                print(f"round {rnd} {cfg} steps {warm + 1}-{warm + K} {name:9s} {us:8.3f} us/step  "
                      f"append {st.get('append_steps', 0)} rebuild {st.get('rebuild_steps', 0)}", flush=True)
    for (cfg, warm, K, name), t in res.items():
        print(f"SUMMARY {cfg} steps {warm + 1}-{warm + K} {name:9s} min {min(t):8.3f} max {max(t):8.3f} "
              f"median {sorted(t)[len(t) // 2]:8.3f} us/step  all {' '.join(f'{x:.3f}' for x in t)}")


if __name__ == "__main__":
    main()
