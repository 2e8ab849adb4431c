"""ab_table.py DIR: the table of one A/B session (README.md of this directory).

Reads DIR/<row>_{parent,child}_{1,2,3}.json, the result lines of `bench.py`
(row `bench`) and `scripts/batch_bench.py` (rows `batch`, `impulses`), and
prints per series the three process values of each side (a process's value is
its own median over its reps), the parent's [min, max] widened by max - min on
either side, the median of the child's three values and the verdict.  The
verdict gates the child's median of three: "within" the interval; "outside, on
the fast side" (a rate above it, a time below it: not a miss); "MISS" (a rate
below it, a time above it).  The last column counts the child's processes
that miss on their own."""
import json, sys, statistics as st
D = sys.argv[1]
def load(row, side, k):
    return json.loads(open(f"{D}/{row}_{side}_{k}.json").read().strip().splitlines()[-1])
series = []   # (name, higher_is_better, getter)
series.append(("bench.py body-steps/s", True, "bench", lambda r: r["value"]))
for E in ("1", "1024", "16384", "262144"):
    series.append((f"batch step E={E} env-steps/s", True, "batch", lambda r, E=E: r["batch"][E]["median"]))
series.append(("batch world env-steps/s", True, "batch", lambda r: r["world"]["median"]))
for E in ("1024", "16384"):
    for f in ("impulses_device", "contacts_device", "step_async_1"):
        series.append((f"impulses E={E} {f} s/call", False, "impulses", lambda r, E=E, f=f: r["impulses"][E][f]["median"]))
print("| series | parent 1..3 | child 1..3 | parent [min, max] widened | child median | verdict | child processes that miss |")
print("|---|---|---|---|---|---|---|")
miss = 0
for name, hib, row, get in series:
    p = [get(load(row, "parent", k)) for k in (1, 2, 3)]
    c = [get(load(row, "child", k)) for k in (1, 2, 3)]
    lo, hi = min(p), max(p); s = hi - lo
    cm = st.median(c)
    ok = (cm >= lo - s) if hib else (cm <= hi + s)
    inside = lo - s <= cm <= hi + s
    verdict = "within" if inside else ("outside, on the fast side" if ok else "MISS")
    miss += not ok
    slow = sum((v < lo - s) if hib else (v > hi + s) for v in c)
    fmt = lambda v: f"{v:.4g}"
    print(f"| {name} | {', '.join(map(fmt, p))} | {', '.join(map(fmt, c))} | [{fmt(lo - s)}, {fmt(hi + s)}] | {fmt(cm)} | {verdict} | {slow} of 3 |")
print(f"\nmisses: {miss}")
