"""Benchmark: body-steps/s of the rigid-body hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c3] [--dtype f64]
                    [--scaling strong|weak] [--full] [--dump-outputs DIR]
    torchrun --nproc-per-node N bench.py --gpus N ...      (driver, N > 1)

A plain run sets up, warms up, times the K steps and prints the result line.
`--full` adds what the headline figure does not need: `cpu_baseline` and
`accuracy` (one GPU), the per-launch kernel timing run (several GPUs).
`--dump-outputs DIR` writes the state after the last timed step, as a caller
of the timed path reads it (gather_state), to DIR/qpos.npy (n, 7) and
DIR/qvel.npy (n, 6) in the world's precision; the scenes are seeded, so the
same arguments give the same inputs on every run.

Workload: C3 (BASELINE.json configs[2]) in fp64 — 65,536 spheres r 0.1 on
flat ground, e 0.8, mu 0.3, dt 0.01, seeded synthetic initial conditions
(rbhip.scenes.flat_spheres).  That is the scene the north-star
target is quoted on ("≥1M body-steps/sec on a 65 536-sphere scene at
1×MI355X with ≥3.5× at 8 GPUs").  `--config c4` is configs[3] (65,536
spheres on the 0.7 rad incline, friction-dominated, "sharded 8×MI355X"),
c2 configs[1] (4,096 spheres), c5 configs[4] (16,384 cubes).  A "step" is
one reference step of the whole scene (contacts, impulses, integration:
the body loop of multi_sphere_bounce.py:42-92).

Scaling (body-id range shards, positions exchanged every step):
  strong (default)  the SAME scene split over the N ranks: rank r owns body
                    ids [r*S, r*S+S), S = ceil(N_bodies / N) — for C3 a slab
                    of 256/N grid rows.  This is the north-star's "≥3.5× at
                    8 GPUs" on one 65,536-sphere scene; N = 1 is the BENCH line.
  weak              N patches of the config side by side on one shared
                    ground, one per rank (per-GPU work fixed).
The ranks exchange positions inside the library, peer-to-peer over xGMI,
in one of two modes: halo pushes (each step, each rank pushes to each
peer only its bodies within a cell of the peer's bounds) or full slice
reads (each step).  Each is warmed up, validated and timed over 20 steps on the node itself;
the fastest valid one runs the timed region
(`config.exchange_probe_ms_per_step` lists them).  RCCL is the fallback
when none validates.

N > 1 is validated: after the warmup and again after the timed region, every
rank's bodies must be bit-identical (compared as uint64 words, so the sign
of zeros counts) to one World of the whole scene stepped the same number of
steps on rank 0's GPU.  A mode that fails the first check (or times out) is
dropped; a failure of the second makes the run exit non-zero instead of
printing a number.

value = total bodies x K / (max over ranks of the timed region), with the
state resident in HBM.  The timed steps are steps D+K+1 .. D+2K from t = 0,
D = W (+20 probe steps for N > 1); the K steps before them capture the
K-step graph: `timed_steps`.
roofline: algorithmic HBM bytes of the step kernel (248 B per
sphere body-step in fp64) x owned bodies / its average launch duration.
One rank: HIP events recorded on the world's stream (torch's current
stream) around the timed region, which is exactly K graph-replayed
step-kernel launches, / K.  Several ranks (--full): an event pair around each
step-kernel launch over a second run of K steps.  `traffic` /
`traffic_lower`: the PMC bounds per launch from the committed
profiles/pmc_traffic.json (rocprofv3 FETCH_SIZE / WRITE_SIZE passes of this
command, profiles/collect_pmc.py), named in `traffic_source`;
`traffic_same_build` says whether they were collected on the library build
this run loaded (the file records its hash).
cpu_baseline (--full, rank 0, N = 1): the oracle (C restatement of the reference
arithmetic) over the full single-GPU scene for --cpu-steps steps from t = 0,
on the host-core share (OMP_NUM_THREADS if set, else the affinity mask) and
on one core, with the host's nproc / affinity / CPU model; `reference_loop`
quotes the reference's own Python loop on C2 (scripts/reference_loop.py,
committed JSON profiles/r05/reference_loop_c2.json).  `accuracy`: the
GPU state after the same --cpu-steps steps against that oracle run (BASELINE
metric "CPU-ref max|Δpos|"), and whether the last step's contact lists agree.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "rigidbody-simulation_amd"))

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec (MI355X_MICROARCH.md)
CONFIG_DESC = {
    "c2": "c2 (BASELINE configs[1]): 4096 spheres, flat ground",
    "c3": "c3 (BASELINE configs[2]): 65536 spheres, flat ground",
    "c4": "c4 (BASELINE configs[3]): 65536 spheres, 0.7 rad incline (friction-dominated)",
    "c5": "c5 (BASELINE configs[4]): 16384 cubes, 0.7 rad incline",
}
TILE = {"c2": (64, 64), "c3": (256, 256), "c4": (256, 256), "c5": (128, 128)}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--config", default="c3", choices=["c2", "c3", "c4", "c5"])
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"])
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the CPU baseline and the "
                         "accuracy run against it (one GPU), the per-launch kernel timing run (several GPUs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline / accuracy")
    ap.add_argument("--cpu-steps", type=int, default=200)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the state after the last timed step as DIR/qpos.npy and DIR/qvel.npy")
    return ap.parse_args()


def dump_outputs(path: str, q, v) -> None:
    """The arrays a caller of the timed path receives after its last step
    (ShardedWorld.gather_state: qpos (n, 7), qvel (n, 6)), whole, in the
    world's precision.  C3 in fp64 is 6.8 MB."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, a in (("qpos", q), ("qvel", v)):
        a = np.ascontiguousarray(a)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        np.save(os.path.join(path, name + ".npy"), a)


# per-config World arguments: C4's rows slide into pile-ups after ~550 steps
# with up to 28 sphere partners on a body; a synchronous
# rb_step grows max_partners itself (guarded chunks), the bench's
# graph-replayed steps cannot, so the timed C4 run starts at 32
WORLD_KW = {"c4": {"max_partners": 32}}


def make_scene(cfg: str, P: int, scaling: str):
    """The scene all ranks step together, and its description."""
    from rbhip import scenes
    if scaling == "strong" or P == 1:
        desc = CONFIG_DESC[cfg] + (f", one scene sharded over {P} GPUs (strong scaling)" if P > 1 else "")
        return scenes.make(cfg), desc
    fn = {"c2": scenes.flat_spheres, "c3": scenes.flat_spheres, "c4": scenes.incline_spheres,
          "c5": scenes.incline_cubes}[cfg]
    nx, ny = TILE[cfg]
    return scenes.tiled(fn, P, nx, ny, seed=0), CONFIG_DESC[cfg] + f" per GPU, {P} patches (weak scaling)"


def host_facts() -> dict:
    """The CPU the baseline ran on: nproc, affinity mask size, model name (lscpu)."""
    model = None
    try:
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        for line in out.splitlines():
            if line.lower().startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except (OSError, subprocess.SubprocessError):
        pass
    if model is None:
        try:
            with open("/proc/cpuinfo") as f:
                for line in f:
                    if line.startswith("model name"):
                        model = line.split(":", 1)[1].strip()
                        break
        except OSError:
            pass
    return {"nproc": os.cpu_count(), "affinity": len(os.sched_getaffinity(0)),
            "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "cpu_model": model}


def cpu_baseline(cfg: str, steps: int):
    """Oracle (C restatement of the reference arithmetic) on the single-GPU
    scene, on this GPU's host-core share (OpenMP over bodies) and on one
    core.  Returns (cpu_baseline dict, the multi-core run's final state and
    last-step contacts) — the latter is the accuracy reference."""
    sys.path.insert(0, ROOT)
    from oracle import oracle as O
    sc, _ = make_scene(cfg, 1, "strong")
    osc = O.OracleScene(sc)
    host = host_facts()
    cores = int(host["omp_num_threads"]) if host["omp_num_threads"] else host["affinity"]
    rates, ref = {}, None
    for th in dict.fromkeys((cores, 1)):
        O.set_threads(th)
        t0 = time.perf_counter()
        res = O.step(osc, sc.qpos0, sc.qvel0, steps, record=(th == cores))
        el = time.perf_counter() - t0
        rates[th] = (sc.n * steps / el, el)
        if th == cores:
            ref = res
    base = {"value": rates[cores][0], "unit": "body-steps/s", "cores": cores, "kind": "port",
            "value_1core": rates[1][0], "host": host,
            "sample": f"oracle/rb_oracle.c (C restatement of collision.py/physics_utils.py/"
                      f"multi_sphere_bounce.py arithmetic, bit-identical to the GPU path) on the full {cfg} "
                      f"scene, {sc.n} bodies x {steps} steps from t=0: {cores} OpenMP threads "
                      f"{rates[cores][1]:.1f} s, 1 thread {rates[1][1]:.1f} s"}
    ref_loop = reference_loop_quote()
    if ref_loop:
        base["reference_loop"] = ref_loop
    return base, ref


REFERENCE_LOOP = os.path.join("profiles", "r05", "reference_loop_c2.json")


def reference_loop_quote():
    """The reference's own Python step loop timed in the build container
    (scripts/reference_loop.py; the reference cannot travel to the GPU box),
    quoted from the committed JSON with its source file."""
    path = os.path.join(ROOT, REFERENCE_LOOP)
    try:
        with open(path) as f:
            r = json.load(f)
    except (OSError, ValueError):
        return None
    return {"value": r["body_steps_per_s"], "unit": "body-steps/s", "cores": r["cores"],
            "value_excluding_mj_forward": r["body_steps_per_s_excluding_mj_forward"],
            "config": r["config"], "bodies": r["bodies"], "steps": r["steps"],
            "cpu_model": r["cpu_model"], "nproc": r["nproc"], "source": REFERENCE_LOOP,
            "script": r["script"], "measured_on": "build container (not the GPU box)"}


def _pairs(cnt, par):
    """(body, partner) pairs of a CSR contact list."""
    import numpy as np
    body = np.repeat(np.arange(cnt.size), cnt)
    return set(zip(body.tolist(), par.tolist()))


def accuracy(cfg: str, dtype: str, device: int, steps: int, ref) -> dict:
    """GPU state against the fp64 oracle (BASELINE metric "CPU-ref max|Δpos|";
    the state written at multi_sphere_bounce.py:85-88) from t = 0: at
    `steps` (the cpu_baseline run, `ref`) and, for fp32 (the
    fp32 vs fp64 sweep), also at steps 1, 10 and 100 — max / median relative
    position error and the contact-flip count (body-partner contacts present
    in one run's last-step list and not the other's)."""
    import numpy as np
    import rbhip
    sys.path.insert(0, ROOT)
    from oracle import oracle as O
    sc, _ = make_scene(cfg, 1, "strong")
    osc = O.OracleScene(sc)
    checkpoints = sorted({1, 10, 100, steps} if dtype == "f32" else {steps})
    checkpoints = [c for c in checkpoints if c <= steps]
    rows = []
    qo, vo = sc.qpos0.copy(), sc.qvel0.copy()
    with rbhip.World(sc, device=device, dtype=dtype) as w:
        w.record_contacts(True)
        done = 0
        for c in checkpoints:
            if c == steps:
                q_ref, v_ref, (cnt, par, kin, dis) = ref
            else:
                qo, vo, (cnt, par, kin, dis) = O.step(osc, qo, vo, c - done, record=True)
                q_ref, v_ref = qo, vo
            w.step(c - done)
            done = c
            q, v = w.get_state()
            gc, gp, gk, _ = w.contacts()
            dx = np.linalg.norm(q[:, :3] - q_ref[:, :3], axis=1)
            dv = np.linalg.norm(v - v_ref, axis=1)
            rel_x = dx / np.maximum(np.linalg.norm(q_ref[:, :3], axis=1), 1e-12)
            rel_v = dv / np.maximum(np.linalg.norm(v_ref, axis=1), 1e-12)
            flips = len(_pairs(gc, gp) ^ _pairs(cnt, par))
            rows.append({"step": c, "max_abs_dpos": float(np.abs(q[:, :3] - q_ref[:, :3]).max()),
                         "max_rel_dpos": float(rel_x.max()), "median_rel_dpos": float(np.median(rel_x)),
                         "max_rel_dvel": float(rel_v.max()), "contact_flips": flips,
                         "contacts_ref": int(cnt.sum()),
                         "contacts_equal": bool(np.array_equal(gc, cnt) and np.array_equal(gp, par) and
                                                np.array_equal(gk, kin)),
                         "bit_identical": bool(np.array_equal(q.view(np.uint64), q_ref.view(np.uint64)) and
                                               np.array_equal(v.view(np.uint64), v_ref.view(np.uint64)))})
    last = rows[-1]
    out = {"vs": "oracle fp64 (cpu_baseline run), same initial conditions, from t = 0",
           "steps": steps, "dtype": dtype,
           **{k: last[k] for k in ("max_abs_dpos", "max_rel_dpos", "max_rel_dvel", "median_rel_dpos",
                                   "contacts_equal", "bit_identical", "contact_flips")},
           "contacts_last_step": last["contacts_ref"],
           "definition": "rel = |d| / |ref| per body (position 3-vector; velocity 6-vector incl. spin); "
                         "contact_flips = |pairs(gpu) xor pairs(oracle)| of the checkpoint step"}
    if len(rows) > 1:
        out["sweep"] = rows
    return out


class SingleWorldCheck:
    """N > 1: compare every rank's bodies, bit for bit, with one World of the
    whole scene stepped on rank 0's GPU (collective: every rank calls it
    with the same step count)."""

    def __init__(self, scene, dtype, device, rank, P, kw=None):
        self.scene, self.dtype, self.device, self.rank, self.P = scene, dtype, device, rank, P
        self.kw = kw or {}
        self.ref, self.done = None, 0

    def __call__(self, sw, steps_total) -> bool:
        import numpy as np
        import torch
        import torch.distributed as dist
        ok = 1
        try:
            sw.sync()
        except Exception as e:          # an exchange timeout or a device error
            print(f"bench: rank {self.rank}: {e}", file=sys.stderr, flush=True)
            ok = 0
        dev = f"cuda:{self.device}" if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor([ok], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        if not int(t.item()):
            return False
        q, v = sw.gather_state()
        same = 1
        if self.rank == 0:
            import rbhip
            if self.ref is None:
                self.ref = rbhip.World(self.scene, device=self.device, dtype=self.dtype, **self.kw)
            self.ref.step(steps_total - self.done)
            self.done = steps_total
            q1, v1 = self.ref.get_state()
            # as 64-bit words: -0.0 and +0.0 differ
            same = int(np.array_equal(q.view(np.uint64), q1.view(np.uint64)) and
                       np.array_equal(v.view(np.uint64), v1.view(np.uint64)))
            if not same:
                bad = np.flatnonzero(~(np.all(q.view(np.uint64) == q1.view(np.uint64), axis=1) &
                                       np.all(v.view(np.uint64) == v1.view(np.uint64), axis=1)))
                print(f"bench: {bad.size} bodies differ from the single World after {steps_total} steps "
                      f"(first ids {bad[:8].tolist()})", file=sys.stderr, flush=True)
        t = torch.tensor([same], device=dev)
        dist.broadcast(t, src=0)
        return bool(int(t.item()))


def step_kernel_name(stats: dict) -> str:
    """The kernel of a form (rb_world_stats "form" numbering)."""
    from rbhip import _lib
    return _lib.FORM_NAMES.get(stats.get("form"), "?")


def region_form(st0: dict, st1: dict, steps: int):
    """(form, clean) of the timed region, from the counters before and after
    it: the tile form only if it committed every one of the K steps with no
    roll-back; a roll-back inside the region (its steps then
    replayed by the hashed forms) makes the region mixed (clean False: its
    kernel time is not one form's); otherwise the hashed form the world
    steps with."""
    d = lambda k: st1.get(k, 0) - st0.get(k, 0)   # noqa: E731
    if d("tile_rollbacks"):
        return st1.get("hashed_form", st1.get("form")), False
    if d("tile_steps") == steps:
        return 5, True
    return st1.get("hashed_form", st1.get("form")), True


def traffic_from_profiles(cfg: str, dtype: str, P: int, scaling: str, suffix: str = ""):
    """(upper, lower, source) HBM bytes per step-kernel launch from the
    committed PMC summary (profiles/pmc_traffic.json, profiles/collect_pmc.py);
    keyed by config and dtype for one GPU, with a _p<N> suffix for strong
    shards and _tile when the tile form stepped the timed region.  (None, None,
    None, None) when that shape was never collected."""
    rel = os.path.join("profiles", "pmc_traffic.json")
    key = f"{cfg}_{dtype}" if P == 1 or scaling == "weak" else f"{cfg}_{dtype}_p{P}"
    key += suffix
    try:
        with open(os.path.join(ROOT, rel)) as f:
            e = json.load(f).get(key)
    except (OSError, ValueError):
        e = None
    if not e:
        return None, None, None, None
    import hashlib
    lib = os.path.join(ROOT, "rigidbody-simulation_amd", "rbhip", "librbhip.so")
    try:
        with open(lib, "rb") as f:
            same = hashlib.sha256(f.read()).hexdigest()[:16] == e.get("librbhip_sha16")
    except OSError:
        same = False
    return e.get("hbm_bytes_per_launch"), e.get("hbm_bytes_per_launch_lower"), f"{rel}[{key}]", same


def main():
    args = parse()
    import torch
    import torch.distributed as dist

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    P = max(world_size, 1)
    # RBHIP_BENCH_BACKEND=gloo (with RBHIP_SHARD_TRANSPORT=p2p) rehearses the
    # multi-rank path with several ranks sharing the visible GPUs; its
    # numbers are not measurements
    backend = os.environ.get("RBHIP_BENCH_BACKEND", "nccl")
    device = local_rank if backend == "nccl" else local_rank % torch.cuda.device_count()
    torch.cuda.set_device(device)
    if P > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{device}"))
        else:
            dist.init_process_group(backend)
    from rbhip.shard import ShardedWorld

    scene, desc = make_scene(args.config, P, args.scaling)
    check = SingleWorldCheck(scene, args.dtype, device, rank, P, WORLD_KW.get(args.config)) if P > 1 else None
    dev_red = f"cuda:{device}" if backend == "nccl" else "cpu"

    def probe_ms(sw) -> float:
        """Max over ranks of PROBE steps' wall time (barrier on both sides)."""
        sw.sync(); torch.cuda.synchronize(); dist.barrier()
        t0 = time.perf_counter()
        sw.step(PROBE)
        sw.sync(); torch.cuda.synchronize()
        t = torch.tensor([time.perf_counter() - t0], device=dev_red, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()) * 1e3 / PROBE

    # N > 1: both peer-to-peer modes (halo pushes, full slice reads) are
    # warmed up, validated against one World and timed over PROBE steps on
    # this node's xGMI; the faster valid one runs the timed region.  The
    # in-library RCCL exchange is the fallback when neither validates, and
    # torch.distributed's all-gather (host-driven) the last one.
    PROBE = 20
    done = args.warmup
    if P == 1:
        sw = ShardedWorld(scene, dtype=args.dtype, device=device, **WORLD_KW.get(args.config, {}))
        sw.step(args.warmup)
        probes = {}
    else:
        cands, probes = [], {}
        # last resort: torch.distributed's all-gather per step (host-driven)
        for tr, halo in [("p2p", True), ("p2p", False), ("rccl", "auto"), ("nccl", False)]:
            if tr in ("rccl", "nccl") and cands:
                break
            try:
                c = ShardedWorld(scene, dtype=args.dtype, device=device, transport=tr, halo=halo,
                                 **WORLD_KW.get(args.config, {}))
            except Exception as ex:
                if rank == 0:
                    print(f"bench: {tr} unavailable: {ex}", file=sys.stderr, flush=True)
                continue
            name = c.transport + (" halo" if c.halo else " full reads" if c.transport == "p2p" else "")
            c.step(args.warmup)
            if not check(c, args.warmup):
                if rank == 0:
                    print(f"bench: {name} exchange failed validation", file=sys.stderr, flush=True)
                c.world.close()
                continue
            probes[name] = probe_ms(c)
            cands.append((probes[name], name, c))
        if not cands:
            raise SystemExit("bench: every transport failed validation")
        cands.sort(key=lambda t: t[0])
        sw = cands[0][2]
        for _, _, c in cands[1:]:
            c.world.close()
        done = args.warmup + PROBE
    w = sw.world
    sw.sync()

    def barrier_sync():
        torch.cuda.synchronize()
        if P > 1:
            dist.barrier()
            torch.cuda.synchronize()

    sw.step(args.steps)              # capture the K-step graph outside the timed region
    sw.sync()
    barrier_sync()
    st0 = w.stats()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()                      # the library enqueues on torch's current stream
    sw.step(args.steps)
    ev1.record()
    # rb_sync inside the clock: it reads the error word and finishes any work
    # the library resolves at a sync point (a rolled-back / continued chunk),
    # so every one of the K steps is complete and checked before the clock stops
    sw.sync()
    barrier_sync()
    elapsed = time.perf_counter() - t0
    region_ms = ev0.elapsed_time(ev1)
    st1 = w.stats()
    timed = [done + args.steps + 1, done + 2 * args.steps]
    if P > 1:
        t = torch.tensor([elapsed], device=dev_red, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        if not check(sw, done + 2 * args.steps):
            raise SystemExit("bench: the sharded run diverged from the single-World run during the timed steps")
    if args.dump_outputs:
        q_out, v_out = sw.gather_state()     # collective for N > 1
        if rank == 0:
            dump_outputs(args.dump_outputs, q_out, v_out)

    # roofline: average step-kernel launch duration.  One rank: the timed
    # region is exactly K back-to-back step-kernel launches (graph replay),
    # so HIP events around it / K.  Several ranks: a step also runs the
    # exchange, so time each step-kernel launch with its own event pair
    # over a run of its own (--full only).
    if P == 1:
        avg_ms, launches, timing = region_ms / args.steps, args.steps, "HIP events around the timed region / K"
    elif args.full:
        w.kernel_timing(True)
        sw.step(args.steps)
        sw.sync()
        avg_ms, launches = w.kernel_timing(False)
        timing = "HIP event pair around each step-kernel launch (second run of K steps)"
    else:
        avg_ms, launches, timing = None, 0, "not timed (--full times each step-kernel launch over a second run)"
    bytes_per_launch = w.bytes_per_body_step * w.n_owned
    achieved = bytes_per_launch / (avg_ms * 1e-3) / 1e9 if avg_ms else 0.0
    form, clean = region_form(st0, st1, args.steps) if P == 1 else (st1.get("hashed_form", st1.get("form")), True)
    traffic, traffic_lower, traffic_src, traffic_same_build = traffic_from_profiles(
        args.config, args.dtype, P, args.scaling, "_tile" if form == 5 else "")
    if not clean:
        traffic = traffic_lower = traffic_src = None
        timing += "; MIXED region: a roll-back inside it was replayed by the hashed forms"

    value = scene.n * args.steps / elapsed
    line = {
        "metric": "body-steps/sec (N spheres x steps/s)",
        "value": value,
        "unit": "body-steps/s",
        "n_gpus": P,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": args.scaling,
        "vs_baseline": None,
        "dtype": args.dtype,
        "data": "synthetic (seeded rbhip.scenes, SURVEY 8d)",
        "timed_steps": timed,
        "config": {"workload": desc, "bodies_total": scene.n, "bodies_per_gpu": w.n_owned,
                   "parallelism": f"body-range shards x{P}" + (
                       f", {sw.transport}{' halo' if sw.halo else ''} position exchange, graph-replayed"
                       if P > 1 else ""),
                   "timed_steps": timed,
                   "dt": scene.dt, "restitution": scene.restitution, "friction": scene.friction,
                   **({"validated": f"bit-identical (uint64 words) to one World of the whole scene after "
                                    f"{args.warmup} and {done + 2 * args.steps} steps",
                       "exchange_probe_ms_per_step": probes} if P > 1 else {})},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_lower": traffic_lower,
                     "traffic_unit": "HBM bytes per launch (PMC FETCH_SIZE / WRITE_SIZE; upper and lower bound)",
                     "traffic_source": traffic_src,
                     # the counters were collected on this very library build
                     "traffic_same_build": traffic_same_build,
                     "kernel": step_kernel_name({"form": form}),
                     "avg_launch_ms": avg_ms, "launches_timed": launches,
                     "timing": timing,
                     "algorithmic_bytes_per_launch": bytes_per_launch},
    }
    if rank == 0 and P == 1 and args.full and not args.no_cpu_baseline:
        w.close()
        base, ref = cpu_baseline(args.config, args.cpu_steps)
        line["cpu_baseline"] = base
        line["accuracy"] = accuracy(args.config, args.dtype, device, args.cpu_steps, ref)
    if rank == 0:
        print(json.dumps(line), flush=True)
    if P > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
