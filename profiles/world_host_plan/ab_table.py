"""ab_table.py DIR: the table of one A/B session (README.md of this directory;
the method and the verdict are profiles/batch_host_split/ab_table.py's).

Reads DIR/<row>_{parent,child}_{1,2,3}.json, the result lines of `bench.py`
(row `bench`), `scripts/batch_bench.py --envs 1` (row `batch`: its one-world
series) and `create_bench.py` (row `create`), and prints per series the three
process values of each side (a process's value is its own median over its
reps), the parent's [min, max] widened by max - min on either side, the median
of the child's three values and the verdict on that median: "within" the
interval; "outside, on the fast side" (a rate above it, a time below it: not a
miss); "MISS" (a rate below it, a time above it).  The last column counts the
child's processes that miss on their own."""
import json, sys, statistics as st
D = sys.argv[1]
def load(row, side, k):
    return json.loads(open(f"{D}/{row}_{side}_{k}.json").read().strip().splitlines()[-1])
series = [("bench.py body-steps/s", True, "bench", lambda r: r["value"]),
          ("batch_bench.py one world, steps/s", True, "batch", lambda r: r["world"]["median"]),
          ("batch_bench.py one world (after), steps/s", True, "batch", lambda r: r["world_after"]["median"]),
          ("create + first step, 65,536 spheres, s", False, "create", lambda r: r["median"])]
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
