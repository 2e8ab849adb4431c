"""Diagnostic: per-phase cycle stamps of the step kernel (RB_STAMPS build).
Phases: 0 start | 1 after table clear | 2 after broadphase search |
3 after state load + gravity | 4 after contact solves | 5 after position
store + insert | 6 end.  Prints the median / p90 over workgroups.
Shared search (the wide + helper form, RBHIP_HELP_SEARCH=1): the helper wave
finishes the body, so the chain 0 .. 6 is the helper wave's (its own buffer):
0 start | 1, 8, 9, 10 its search | 2 its last hit written | 11 past the
barrier | 7 after the merge and sort | 3 .. 6 as above.  The body wave only
searches: 0, 1, 8, 9, 10, and 2 once it is past the barrier (10 -> 2: its
wait for the helper)."""
import ctypes, os, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rigidbody-simulation_amd"))
CSRC = os.path.join(ROOT, "rigidbody-simulation_amd", "csrc")
extra = os.environ.get("EXTRA_FLAGS", "")
# a prebuilt stamps library (built on the CPU host, shipped with the tree) or build one here
LIB = os.environ.get("STAMP_LIB", "/tmp/libstamp.so")
if not os.path.exists(LIB):
    subprocess.run(["make", "-s", "-C", CSRC, f"EXTRA=-DRB_STAMPS=1 {extra}".strip(), f"OUT={LIB}", "OBJDIR=build/stamps"],
                   check=True)
from rbhip import _lib, scenes
import rbhip.world as W
L = _lib.load(LIB)
L.rb_diag_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]
def report_finish(sc, kind, buf, hbuf):
    """Shared search: the helper (finishing) wave's chain from its start to
    its last store, and the body (search-only) wave beside it."""
    a, h = buf.astype(np.int64), hbuf.astype(np.int64)

    def line(who, t, lo, hi, nm):
        dd = t[:, hi] - t[:, lo]
        print(f"     {who} {nm:24s} median {int(np.median(dd)):8d}  p90 {int(np.percentile(dd, 90)):8d}")

    tot = h[:, 6] - h[:, 0]
    span = h[:, 6].max() - min(h[:, 0].min(), a[:, 0].min())
    print(f"N={sc.n} [{kind} launch, shared search]: kernel span {int(span)} cyc; finishing wave start -> last store "
          f"median {int(np.median(tot))} p90 {int(np.percentile(tot, 90))}")
    for lo, hi, nm in [(0, 1, "lead"), (1, 8, "snap+heads issue+own work"), (8, 9, "heads+batch1"), (9, 10, "later batches"),
                       (10, 2, "last hit written"), (2, 11, "barrier"), (11, 7, "merge+sort"), (7, 3, "force (applied only)"),
                       (3, 4, "solves"), (4, 5, "pos+insert"), (5, 6, "quat+store")]:
        line("finishing", h, lo, hi, nm)
    for lo, hi, nm in [(0, 1, "lead"), (1, 10, "search"), (10, 2, "wait at the barrier")]:
        line("search-only", a, lo, hi, nm)
    late = h[:, 2] - a[:, 10]
    print(f"     search-only wave done before the finishing wave's last hit by median {int(np.median(late))} "
          f"p90 {int(np.percentile(late, 90))}")


def report(sc, G, kind, buf):
    d = np.diff(buf[:, :7].astype(np.int64), axis=1)
    tot = (buf[:, 6].astype(np.int64) - buf[:, 0].astype(np.int64))
    span = buf[:, 6].max() - buf[:, 0].min()
    print(f"N={sc.n} [{kind} launch]: kernel span {int(span)} cyc; per-block total median {int(np.median(tot))} p90 {int(np.percentile(tot, 90))}")
    names = ["clear", "search", "load+grav", "solves", "pos+insert", "quat+store"]
    for k, nm in enumerate(names):
        print(f"   {nm:12s} median {int(np.median(d[:, k])):8d}  p90 {int(np.percentile(d[:, k], 90)):8d}")
    if G == 1:  # one-lane search sub-phases
        sub = [(1, 8, "snap+heads issue"), (8, 9, "heads+batch1"), (9, 10, "later batches"), (10, 2, "tail")]
        for a, b_, nm in sub:
            dd = buf[:, b_].astype(np.int64) - buf[:, a].astype(np.int64)
            print(f"     {nm:16s} median {int(np.median(dd)):8d}  p90 {int(np.percentile(dd, 90)):8d}")
    if G > 1:   # cooperative search sub-phases
        sub = [(1, 8, "snap+cell"), (8, 9, "invI"), (9, 10, "bucket+test"), (10, 11, "place+sync"), (11, 2, "sort+sync")]
        for a, b_, nm in sub:
            dd = buf[:, b_].astype(np.int64) - buf[:, a].astype(np.int64)
            print(f"     {nm:12s} median {int(np.median(dd)):8d}  p90 {int(np.percentile(dd, 90)):8d}")


sizes = [(64, 64, 300), (256, 256, 60), (1024, 1024, 60)]
if os.environ.get("STAMP_SIZES"):        # e.g. "64x64,128x64,256x256"
    sizes = [(int(a), int(b), 300) for a, b in (t.split("x") for t in os.environ["STAMP_SIZES"].split(","))]
for nx, ny, warm in sizes:
    if nx * ny * (8 if nx * ny <= 20480 else 1) > 64 * (1 << 16): continue
    sc = scenes.flat_spheres(nx, ny, seed=0)
    G = 8 if sc.n <= int(os.environ.get("RBHIP_COOP_MAX_BODIES", "20480")) else 1
    nb = (sc.n * G + 63) // 64
    # worlds with append epochs: the first append launch and the
    # first rebuild launch after the warm-up, each reported on its own (told
    # apart by the counters); other worlds: the launch after the warm-up
    seen = {}
    with W.World(sc) as w:
        w.step(warm)
        for _ in range(2 * w.stats().get("table_epoch", 1) + 2):
            st0 = w.stats()
            w.step(1)
            st1 = w.stats()
            kind = ("append" if st1.get("append_steps", 0) > st0.get("append_steps", 0)
                    else "rebuild" if st1.get("rebuild_steps", 0) > st0.get("rebuild_steps", 0) else "step")
            if kind not in seen:
                buf = np.zeros((nb, 16), np.uint64)
                L.rb_diag_stamps(buf.ctypes.data_as(ctypes.c_void_p), nb)
                hbuf = np.zeros((nb, 16), np.uint64)
                if hasattr(L, "rb_diag_stamps_help"):
                    L.rb_diag_stamps_help.argtypes = [ctypes.c_void_p, ctypes.c_int]
                    L.rb_diag_stamps_help(hbuf.ctypes.data_as(ctypes.c_void_p), nb)
                seen[kind] = (buf, hbuf)
            if kind == "step" or len(seen) == 2:
                break
    for kind, (buf, hbuf) in seen.items():
        if G == 1 and hbuf[:, 6].any():           # the helper wave reached the end: it finished the bodies
            report_finish(sc, kind, buf, hbuf)
        else:
            report(sc, G, kind, buf)
