#!/usr/bin/env python
"""Environment-steps per second of batched worlds (rbhip.BatchWorld) against
one World stepping the same scene.

The scene is the reference's multi_sphere4 (models/multi_sphere.xml: four
balls) in f64.  A batch of E environments runs a restitution sweep
(sim_overrides.py's knob, 0.5 .. 1.0 over the environments); every timed
window is `--steps` steps around one synchronous step call, after a warm-up
of the same length, from the same start state, repeated `--reps` times so the
spread is visible.  In the same run one World(multi_sphere4) steps `--steps`
steps the same number of times: without batches that is the only way to run
the scene, one World call per environment.

--law balls: the same measurement on the reference's ball_collision scene
(two balls, the two-ball law) against one World(law="balls").

--sampled EVERY: instead, the time of run_sampled(steps, EVERY) against the
loop it replaces, step(EVERY) + get_state() per sample, on the same batch and
start state (seconds per run; bytes sampled per second next to it).

--per-env: next to the plain run of every E, in the same process and
alternating rep by rep, the same sweep through the per-environment (ENVS)
instance of the step kernel: every environment's planes and gravity set to
the template's values and an all-zero xfrc (set_planes / set_gravity /
set_xfrc), and once more with planes and gravity only (with forces set every
body takes the applied-force path, which inverts the world inertia every
step).  Adds "batch_env", "batch_env_no_xfrc", "env_over_plain" and
"env_no_xfrc_over_plain" to the JSON line.  (The environment counts already
own the name --envs.)

--incline-sweep N: instead, N cube-incline angles (scenes.cube_incline, 0 ..
0.7 rad) as one batch (BatchWorld.from_scenes) against N one-environment
batches stepped one after another, the only way to run the sweep in batches
without per-environment planes; f64 only, seconds per `--steps` steps.

--box-pile NX,NY,LAYERS: the same measurement on scenes.box_pile(NX, NY,
LAYERS) (columns of cubes, some capped with a sphere: box-involved pairs, the
mixed-template kernel) with a friction sweep (0.2 .. 0.8 over the
environments) against one World(scene, max_partners=32).

--wide-pile NX,NY,LAYERS: --box-pile for a pile of 65 to 256 bodies, which is
a wide batch (one environment per workgroup of 2 to 4 waves), against one
World(scene, max_partners=32), the most a world takes: box_pile(4, 4, 4) is 70
bodies, box_pile(8, 8, 3) 214.

--device-loop K: instead, a closed loop's iteration (new applied forces, K
steps, read the state, reset 1 % of the environments) through the
device-resident boundary (set_xfrc_device, step_async(K), get_state_device,
set_state_device(mask); torch tensors on the batch's stream, one sync() at the
end of the timed window) against the same iteration through host arrays
(set_xfrc, step(K), get_state, set_state(envs=...)) on the same batch,
alternating; `--steps` iterations per window, seconds per iteration.

--sampled-device EVERY: run_sampled_device(steps, EVERY) into tensors
allocated once, with its sync(), against run_sampled(steps, EVERY) on the
same batch, alternating; seconds per run, and the ratio to the same steps
unsampled.

--contacts R: instead, the contact query with R records per body on a batch
that has stepped `--steps` steps: contacts_device(R) per call (tensors
allocated once, 20 calls and one sync() per window) against one step_async(1)
of the same batch, and the host form contacts(R) against get_state(),
alternating; seconds per call.  With --box-pile NX,NY,LAYERS the scene is that
pile (the mixed-template instance of the query's kernel).

--impulses R: instead, the impulse query with R records per body (0: the
"sensor only" call) on a batch that has stepped `--steps` steps:
impulses_device(R) per call (tensors allocated once, 20 calls and one sync()
per window) against one step_async(1) and against contacts_device(R, without
geometry) of the same batch, alternating; seconds per call.  With --box-pile
NX,NY,LAYERS the scene is that pile (the box instances of the query's
kernel).  Writes to profiles/batch_impulses/ unless --out is given.

--sampled-impulses EVERY: instead, the contact-impulse curves of a sampled run:
run_sampled_impulses_device(steps, EVERY) with all three outputs and with net
alone against run_sampled_device(steps, EVERY) of the same run, alternating,
device tensors allocated once, one sync() per run (seconds per run; the ratios
are what sensing costs inside the step loop).  With EVERY 1 also the loop the
call replaces: impulses_device(max_records=0) + step_async(1) per step.  The
environments run a friction sweep (0.2 .. 0.8); --box-pile selects the scene.
Writes profiles/batch_sampled_impulses/sensed_<scene>_every<EVERY>.json.

--ragged LO,HI: instead, an ensemble of E scenes whose body counts are spread
evenly over LO..HI (--ragged-scene flat_spheres: rows of spheres; box_pile:
columns of two cubes, the first n bodies), f64.  Three measurements in one
process, alternating rep by rep: (1) the ensemble as one batch with a
population (BatchWorld.from_ragged_scenes: the lanes packed by body count);
(2) what had to be done without populations: one uniform batch per distinct
body count, stepped one after another, times summed; (3) for a uniform
ensemble (all counts HI), a batch with the uniform population set (the ragged
kernels) against the same batch with none (the kernels of a batch without
population): the price of the tables and the per-environment kinds.
"packed_over_unpacked" is (1) over the ragged rate of (3): the ragged kernels
on E x HI lanes' worth of work, what the ensemble would cost with the fixed
mapping.  Writes to profiles/batch_ragged/ unless --out is given.

Prints one JSON line and writes it to --out (default
profiles/batch/batch_bench.json).  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rigidbody-simulation_amd"))


def _summary(rates):
    r = sorted(rates)
    return dict(median=r[len(r) // 2], min=r[0], max=r[-1], reps=rates)


def _batch(rb, sc, E, dtype, law):
    # (the default law through the constructor every version of the library has)
    return rb.BatchWorld(sc, E, dtype=dtype) if law == "mujoco" else rb.BatchWorld(sc, E, dtype=dtype, law=law)


def bench_batch(rb, sc, E, steps, reps, dtype, law="mujoco", sweep=None):
    """sweep: the per-environment knob, {name: (lo, hi)} (default: restitution 0.5 .. 1.0)"""
    sweep = sweep or {"restitution": (0.5, 1.0)}
    q = np.broadcast_to(sc.qpos0, (E, sc.n, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (E, sc.n, 6)).copy()
    with _batch(rb, sc, E, dtype, law) as b:
        b.set_params(**{k: np.linspace(lo, hi, E) for k, (lo, hi) in sweep.items()})
        b.step(steps)                                   # warm-up
        rates = []
        for _ in range(reps):
            b.set_state(q, v)
            t0 = time.perf_counter()
            failed = b.step(steps)                      # synchronous
            dt = time.perf_counter() - t0
            if failed:
                raise RuntimeError(f"{failed} environments failed")
            rates.append(E * steps / dt)
    return _summary(rates)


def bench_batch_env(rb, sc, E, steps, reps, dtype):
    """The plain instance and the ENVS instance on the same sweep, alternating
    rep by rep in one process: three batches of the same start state, one
    plain, one with per-environment planes and gravity equal to the
    template's and a zero xfrc, one with those planes and gravity only."""
    q = np.broadcast_to(sc.qpos0, (E, sc.n, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (E, sc.n, 6)).copy()
    with rb.BatchWorld(sc, E, dtype=dtype) as plain, rb.BatchWorld(sc, E, dtype=dtype) as env, \
            rb.BatchWorld(sc, E, dtype=dtype) as env_nx:
        for b in (env, env_nx):
            b.set_planes(sc.planes)
            b.set_gravity(sc.gravity)
        env.set_xfrc(np.zeros(6))
        rates = {"plain": [], "env": [], "env_nx": []}
        for b in (plain, env, env_nx):
            b.set_params(restitution=np.linspace(0.5, 1.0, E))
            b.step(steps)                               # warm-up
        for _ in range(reps):
            for name, b in (("plain", plain), ("env", env), ("env_nx", env_nx)):
                b.set_state(q, v)
                t0 = time.perf_counter()
                failed = b.step(steps)
                dt = time.perf_counter() - t0
                if failed:
                    raise RuntimeError(f"{failed} environments failed")
                rates[name].append(E * steps / dt)
    return _summary(rates["plain"]), _summary(rates["env"]), _summary(rates["env_nx"])


def bench_incline_sweep(rb, n, steps, reps):
    """n cube-incline angles: one batch of n environments against n batches of
    one environment stepped one after another, alternating; seconds per run."""
    from rbhip import scenes
    scs = [scenes.cube_incline(0.7 * k / max(n - 1, 1)) for k in range(n)]
    q = np.stack([sc.qpos0 for sc in scs])
    v = np.stack([sc.qvel0 for sc in scs])
    ones = [rb.BatchWorld(sc, 1) for sc in scs]
    try:
        with rb.BatchWorld.from_scenes(scs) as sweep:
            sweep.step(steps)                           # warm-up of both
            for b in ones:
                b.step(steps)
            t_sweep, t_ones = [], []
            for _ in range(reps):
                sweep.set_state(q, v)
                t0 = time.perf_counter()
                sweep.step(steps)
                t_sweep.append(time.perf_counter() - t0)
                for k, b in enumerate(ones):
                    b.set_state(q[k:k + 1], v[k:k + 1])
                t0 = time.perf_counter()
                for b in ones:
                    b.step(steps)
                t_ones.append(time.perf_counter() - t0)
            sq, sv = sweep.get_state()
            same = all(np.array_equal(np.concatenate(b.get_state(), axis=2).view(np.uint64),
                                      np.concatenate([sq[k:k + 1], sv[k:k + 1]], axis=2).view(np.uint64))
                       for k, b in enumerate(ones))
    finally:
        for b in ones:
            b.close()
    out = dict(angles=n, identical=bool(same), one_batch_s=_summary(t_sweep), n_batches_s=_summary(t_ones))
    out["speedup_median"] = out["n_batches_s"]["median"] / out["one_batch_s"]["median"]
    return out


def bench_sampled(rb, sc, E, steps, every, reps, dtype, law="mujoco"):
    """Seconds per run of run_sampled(steps, every) and of the loop it
    replaces, alternating, from the same start state; the two must return the
    same words."""
    q = np.broadcast_to(sc.qpos0, (E, sc.n, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (E, sc.n, 6)).copy()
    S = steps // every

    def loop(b):
        sq = np.zeros((S, E, sc.n, 7))
        sv = np.zeros((S, E, sc.n, 6))
        for s in range(S):
            b.step(every)
            sq[s], sv[s] = b.get_state()
        b.step(steps - S * every)
        return sq, sv

    with _batch(rb, sc, E, dtype, law) as b:
        b.set_params(restitution=np.linspace(0.5, 1.0, E))
        b.set_state(q, v)
        lq, lv = loop(b)                                # warm-up of both, and the comparison
        b.set_state(q, v)
        sq, sv, _ = b.run_sampled(steps, every)
        same = bool(np.array_equal(sq.view(np.uint64), lq.view(np.uint64)) and
                    np.array_equal(sv.view(np.uint64), lv.view(np.uint64)))
        del lq, lv, sq, sv
        t_loop, t_samp = [], []
        for _ in range(reps):
            b.set_state(q, v)
            t0 = time.perf_counter()
            loop(b)
            t_loop.append(time.perf_counter() - t0)
            b.set_state(q, v)
            t0 = time.perf_counter()
            b.run_sampled(steps, every)
            t_samp.append(time.perf_counter() - t0)
        t_plain = []
        for _ in range(reps):
            b.set_state(q, v)
            t0 = time.perf_counter()
            b.step(steps)
            t_plain.append(time.perf_counter() - t0)
    nbytes = S * E * sc.n * 13 * 8                      # what reaches the caller
    out = dict(samples=S, bytes=nbytes, identical=same, loop_s=_summary(t_loop), sampled_s=_summary(t_samp),
               step_only_s=_summary(t_plain))
    out["sampled_bytes_per_s"] = nbytes / out["sampled_s"]["median"] if S else 0.0
    out["loop_bytes_per_s"] = nbytes / out["loop_s"]["median"] if S else 0.0
    out["speedup_median"] = out["loop_s"]["median"] / out["sampled_s"]["median"]
    out["slowest_sampled_beats_fastest_loop"] = out["sampled_s"]["max"] < out["loop_s"]["min"]
    return out


def _words(a):
    return np.ascontiguousarray(a).view(np.uint64)


def bench_device_loop(rb, sc, E, K, iters, reps, dtype):
    """Seconds per iteration of the closed loop through device tensors and
    through host arrays, alternating, from the same start state; the final
    states must agree word for word in every repeat."""
    import torch
    rng = np.random.default_rng(0)
    q = np.broadcast_to(sc.qpos0, (E, sc.n, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (E, sc.n, 6)).copy()
    xf = np.concatenate([rng.normal(0.0, 0.5, (E, sc.n, 3)), rng.normal(0.0, 0.05, (E, sc.n, 3))], axis=2)
    mask = np.zeros(E, bool)
    mask[::100] = True                                  # 1 % of the environments are reset every iteration
    ids = np.nonzero(mask)[0]
    rq, rv = q[ids].copy(), v[ids].copy()
    with rb.BatchWorld(sc, E, dtype=dtype) as b:
        b.set_params(restitution=np.linspace(0.5, 1.0, E))
        b.use_stream(torch.cuda.current_stream().cuda_stream)
        dev = f"cuda:{b.device}"
        xf_d, q_d, v_d, mask_d = (torch.from_numpy(a).to(dev) for a in (xf, q, v, mask))
        out_q, out_v = torch.empty_like(q_d), torch.empty_like(v_d)

        def device_loop(n):
            for _ in range(n):
                b.set_xfrc_device(xf_d)
                b.step_async(K)
                b.get_state_device(out_q, out_v)
                b.set_state_device(q_d, v_d, mask=mask_d)
            if b.sync():
                raise RuntimeError("environments failed")

        def host_loop(n):
            for _ in range(n):
                b.set_xfrc(xf)
                if b.step(K):
                    raise RuntimeError("environments failed")
                b.get_state()
                b.set_state(rq, rv, envs=ids)

        b.set_state(q, v)
        device_loop(3)                                  # warm-up of both
        host_loop(3)
        t_dev, t_host, same = [], [], True
        for _ in range(reps):
            b.set_state(q, v)
            t0 = time.perf_counter()
            device_loop(iters)
            t_dev.append((time.perf_counter() - t0) / iters)
            dq, dv = b.get_state()
            b.set_state(q, v)
            t0 = time.perf_counter()
            host_loop(iters)
            t_host.append((time.perf_counter() - t0) / iters)
            hq, hv = b.get_state()
            same = same and bool(np.array_equal(_words(dq), _words(hq)) and np.array_equal(_words(dv), _words(hv)))
    out = dict(iterations=iters, identical=same, device_s=_summary(t_dev), host_s=_summary(t_host))
    out["speedup_median"] = out["host_s"]["median"] / out["device_s"]["median"]
    out["slowest_device_beats_fastest_host"] = out["device_s"]["max"] < out["host_s"]["min"]
    return out


def bench_sampled_device(rb, sc, E, steps, every, reps, dtype):
    """Seconds per run of run_sampled_device(steps, every) + sync() and of
    run_sampled(steps, every), alternating, from the same start state; the two
    must return the same words."""
    import torch
    q = np.broadcast_to(sc.qpos0, (E, sc.n, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (E, sc.n, 6)).copy()
    S = steps // every
    with rb.BatchWorld(sc, E, dtype=dtype) as b:
        b.set_params(restitution=np.linspace(0.5, 1.0, E))
        b.use_stream(torch.cuda.current_stream().cuda_stream)
        dev = f"cuda:{b.device}"
        out_q = torch.empty((S, E, sc.n, 7), dtype=torch.float64, device=dev)
        out_v = torch.empty((S, E, sc.n, 6), dtype=torch.float64, device=dev)
        b.set_state(q, v)
        hq, hv, _ = b.run_sampled(steps, every)         # warm-up of both, and the comparison
        b.set_state(q, v)
        b.run_sampled_device(steps, every, out_qpos=out_q, out_qvel=out_v)
        b.sync()
        same = bool(np.array_equal(_words(out_q.cpu().numpy()), _words(hq)) and
                    np.array_equal(_words(out_v.cpu().numpy()), _words(hv)))
        del hq, hv
        t_dev, t_host, t_plain = [], [], []
        for _ in range(reps):
            b.set_state(q, v)
            t0 = time.perf_counter()
            b.run_sampled_device(steps, every, out_qpos=out_q, out_qvel=out_v)
            b.sync()
            t_dev.append(time.perf_counter() - t0)
            b.set_state(q, v)
            t0 = time.perf_counter()
            b.run_sampled(steps, every)
            t_host.append(time.perf_counter() - t0)
            b.set_state(q, v)
            t0 = time.perf_counter()
            b.step(steps)
            t_plain.append(time.perf_counter() - t0)
    nbytes = S * E * sc.n * 13 * 8
    out = dict(samples=S, bytes=nbytes, identical=same, device_s=_summary(t_dev), host_s=_summary(t_host),
               step_only_s=_summary(t_plain))
    out["device_bytes_per_s"] = nbytes / out["device_s"]["median"] if S else 0.0
    out["speedup_median"] = out["host_s"]["median"] / out["device_s"]["median"]
    out["device_over_step_only"] = out["device_s"]["median"] / out["step_only_s"]["median"]
    out["slowest_device_beats_fastest_host"] = out["device_s"]["max"] < out["host_s"]["min"]
    return out


def bench_contacts(rb, sc, E, R, settle, reps, dtype, calls=20):
    """Seconds per call of the contact query on a batch that has stepped
    `settle` steps: contacts_device(R) into tensors allocated once against one
    step_async(1) (each `calls` calls and one sync() per window), and the host
    form contacts(R) against get_state(), alternating."""
    import torch
    with rb.BatchWorld(sc, E, dtype=dtype) as b:
        b.set_params(restitution=np.linspace(0.5, 1.0, E))
        b.use_stream(torch.cuda.current_stream().cuda_stream)
        if b.step(settle):
            raise RuntimeError("environments failed")
        out = b.contacts_device(max_records=R)
        b.sync()
        host = b.contacts(max_records=R)                # warm-up of both, and the comparison
        same = bool(all(np.array_equal(getattr(out, f).cpu().numpy(), getattr(host, f))
                        for f in ("counts", "partner", "kind", "dist", "pos", "frame")))
        listed = int(np.maximum(host.counts, 0).sum())
        q0, v0 = b.get_state()
        t = {"contacts_device": [], "step_async_1": [], "contacts_host": [], "get_state": []}

        def window(name, f, n):
            t0 = time.perf_counter()
            for _ in range(n):
                f()
            b.sync()
            t[name].append((time.perf_counter() - t0) / n)

        for _ in range(reps):
            window("contacts_device", lambda: b.contacts_device(out=out), calls)
            b.set_state(q0, v0)
            window("step_async_1", lambda: b.step_async(1), calls)
            b.set_state(q0, v0)
            window("contacts_host", lambda: b.contacts(max_records=R), 1)
            window("get_state", b.get_state, 1)
    res = dict(max_records=R, settle_steps=settle, calls_per_window=calls, contacts_listed=listed,
               truncated=host.truncated, identical=same, **{k: _summary(v) for k, v in t.items()})
    res["device_over_step"] = res["contacts_device"]["median"] / res["step_async_1"]["median"]
    res["host_over_get_state"] = res["contacts_host"]["median"] / res["get_state"]["median"]
    return res


def bench_impulses(rb, sc, E, R, settle, reps, dtype, calls=20):
    """Seconds per call of the impulse query on a batch that has stepped
    `settle` steps: impulses_device(R) into tensors allocated once against one
    step_async(1) and against contacts_device(R) without geometry (each `calls`
    calls and one sync() per window), alternating; the host form once, for the
    comparison of the two forms."""
    import torch
    with rb.BatchWorld(sc, E, dtype=dtype) as b:
        b.set_params(restitution=np.linspace(0.5, 1.0, E))
        b.use_stream(torch.cuda.current_stream().cuda_stream)
        if b.step(settle):
            raise RuntimeError("environments failed")
        out = b.impulses_device(max_records=R)
        con = b.contacts_device(max_records=R, geometry=False)
        b.sync()
        host = b.impulses(max_records=R)                # warm-up, and the comparison
        fields = ("counts", "vel", "net") + (("partner", "kind", "dist", "jn", "jt") if R > 0 else ())
        same = bool(all(np.array_equal(getattr(out, f).cpu().numpy(), getattr(host, f)) for f in fields))
        listed = int(np.maximum(host.counts, 0).sum())
        applied = int((host.jn != 0).sum()) if R > 0 else None
        q0, v0 = b.get_state()
        t = {"impulses_device": [], "contacts_device": [], "step_async_1": []}

        def window(name, f, n):
            t0 = time.perf_counter()
            for _ in range(n):
                f()
            b.sync()
            t[name].append((time.perf_counter() - t0) / n)

        for _ in range(reps):
            window("impulses_device", lambda: b.impulses_device(out=out), calls)
            window("contacts_device", lambda: b.contacts_device(out=con), calls)
            window("step_async_1", lambda: b.step_async(1), calls)
            b.set_state(q0, v0)
    res = dict(max_records=R, settle_steps=settle, calls_per_window=calls, contacts_listed=listed, nonzero_jn=applied,
               truncated=host.truncated, identical=same, **{k: _summary(v) for k, v in t.items()})
    res["impulses_over_step"] = res["impulses_device"]["median"] / res["step_async_1"]["median"]
    res["impulses_over_contacts"] = res["impulses_device"]["median"] / res["contacts_device"]["median"]
    return res


def bench_sampled_impulses(rb, sc, E, steps, every, reps, dtype):
    """Seconds per run, from the same start state, alternating, all through
    device tensors allocated once and one sync() per run:
    run_sampled_impulses_device(steps, every) with all three outputs and with
    net alone, against run_sampled_device(steps, every) of the same run (what
    sensing costs inside the loop); with every == 1 also the loop it replaces,
    impulses_device(max_records=0) + step_async(1) per step.  The friction of
    the environments is spread over 0.2 .. 0.8.  The net rows of the call and
    of the loop must be the same words."""
    import torch
    q = np.broadcast_to(sc.qpos0, (E, sc.n, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (E, sc.n, 6)).copy()
    S = steps // every
    with rb.BatchWorld(sc, E, dtype=dtype) as b:
        b.set_params(friction=np.linspace(0.2, 0.8, E))
        b.use_stream(torch.cuda.current_stream().cuda_stream)
        dev = f"cuda:{b.device}"
        out_q = torch.empty((S, E, sc.n, 7), dtype=torch.float64, device=dev)
        out_v = torch.empty((S, E, sc.n, 6), dtype=torch.float64, device=dev)
        out_n = torch.empty((S, E, sc.n, 6), dtype=torch.float64, device=dev)
        loop_n = torch.empty((S, E, sc.n, 6), dtype=torch.float64, device=dev) if every == 1 else None
        counts = torch.empty((E, sc.n), dtype=torch.int32, device=dev)

        def full():
            b.run_sampled_impulses_device(steps, every, out_qpos=out_q, out_qvel=out_v, out_net=out_n)

        def net_only():
            b.run_sampled_impulses_device(steps, every, positions=False, velocities=False, out_net=out_n)

        def plain():
            b.run_sampled_device(steps, every, out_qpos=out_q, out_qvel=out_v)

        def loop():
            for s in range(steps):
                b.impulses_device(max_records=0, out=dict(counts=counts, net=loop_n[s]))
                b.step_async(1)

        runs = dict(sensed_all=full, sensed_net_only=net_only, run_sampled_device=plain)
        if every == 1:
            runs["impulses_step_loop"] = loop
        t = {k: [] for k in runs}
        words = {}
        for k, f in runs.items():                       # warm-up of each, and the comparison
            b.set_state(q, v)
            f()
            failed = b.sync()
            if k != "run_sampled_device":
                words[k] = (loop_n if k == "impulses_step_loop" else out_n).cpu().numpy().view(np.uint64).copy()
        same = all(np.array_equal(w, words["sensed_all"]) for w in words.values())
        nonzero = int((words["sensed_all"] & 0x7fffffffffffffff != 0).any(axis=-1).sum())
        del words
        for _ in range(reps):
            for k, f in runs.items():
                b.set_state(q, v)
                t0 = time.perf_counter()
                f()
                b.sync()
                t[k].append(time.perf_counter() - t0)
    res = dict(samples=S, every=every, failed=failed, net_identical=bool(same), nonzero_net_rows=nonzero,
               **{k: _summary(x) for k, x in t.items()})
    base = res["run_sampled_device"]["median"]
    res["sensed_all_over_run_sampled"] = res["sensed_all"]["median"] / base
    res["sensed_net_only_over_run_sampled"] = res["sensed_net_only"]["median"] / base
    if every == 1:
        res["loop_over_sensed_net_only"] = res["impulses_step_loop"]["median"] / res["sensed_net_only"]["median"]
        res["loop_over_sensed_all"] = res["impulses_step_loop"]["median"] / res["sensed_all"]["median"]
    return res


def ragged_scene(variant, n, seed):
    """A scene of n bodies: a row of spheres, or the first n bodies of columns of two cubes."""
    from rbhip import scenes
    if variant == "flat_spheres":
        return scenes.flat_spheres(n, 1, seed=seed, spacing=0.19)
    sc = scenes.box_pile((n + 1) // 2, 1, 2, seed=seed, sphere_every=0)
    return sc.with_(kind=sc.kind[:n], mass=sc.mass[:n], inertia=sc.inertia[:n], size=sc.size[:n], qpos0=sc.qpos0[:n],
                    qvel0=sc.qvel0[:n])


def bench_ragged(rb, variant, lo, hi, E, steps, reps, seeds=16):
    """Environment-steps per second of (1) the ragged ensemble as one batch,
    (2) one uniform batch per distinct body count, stepped one after another,
    (3) a uniform ensemble of hi bodies with and without a population;
    alternating rep by rep in one process."""
    counts = [lo + k % (hi - lo + 1) for k in range(E)]
    cache = {}

    def scene(n, k):
        key = (n, k % seeds)
        if key not in cache:
            cache[key] = ragged_scene(variant, n, k % seeds)
        return cache[key]

    scs = [scene(n, k) for k, n in enumerate(counts)]
    groups = {n: [sc for sc in scs if sc.n == n] for n in sorted(set(counts))}
    full = [scene(hi, k) for k in range(E)]
    rates = {"ragged": [], "per_shape": [], "uniform_plain": [], "uniform_ragged": []}

    def timed(b, q, v):
        b.set_state(q, v)
        t0 = time.perf_counter()
        failed = b.step(steps)                          # synchronous
        dt = time.perf_counter() - t0
        if failed:
            raise RuntimeError(f"{failed} environments failed")
        return dt

    def state(b):
        return b.get_state()

    shapes = [rb.BatchWorld.from_scenes(g) for g in groups.values()]
    try:
        with rb.BatchWorld.from_ragged_scenes(scs) as ragged, rb.BatchWorld.from_scenes(full) as plain, \
                rb.BatchWorld.from_scenes(full) as uni:
            uni.set_population(np.full(E, hi), np.tile(full[0].kind, (E, 1)))
            every = [ragged, plain, uni] + shapes
            start = [state(b) for b in every]           # the initial states, before the warm-up
            for b in every:
                b.step(steps)                           # warm-up
            for _ in range(reps):
                rates["ragged"].append(E * steps / timed(ragged, *start[0]))
                rates["per_shape"].append(E * steps / sum(timed(b, *st) for b, st in zip(shapes, start[3:])))
                rates["uniform_plain"].append(E * steps / timed(plain, *start[1]))
                rates["uniform_ragged"].append(E * steps / timed(uni, *start[2]))
            same = bool(np.array_equal(_words(plain.get_state()[0]), _words(uni.get_state()[0])))
    finally:
        for b in shapes:
            b.close()
    out = {k: _summary(v) for k, v in rates.items()}
    out.update(present_bodies=int(sum(counts)), lanes_fixed_mapping=E * hi, distinct_shapes=len(groups),
               uniform_identical=same)
    out["ragged_over_per_shape"] = out["ragged"]["median"] / out["per_shape"]["median"]
    out["uniform_ragged_over_plain"] = out["uniform_ragged"]["median"] / out["uniform_plain"]["median"]
    out["packed_over_unpacked"] = out["ragged"]["median"] / out["uniform_ragged"]["median"]
    return out


def bench_world(rb, sc, steps, reps, dtype, law="mujoco", **kw):
    with (rb.World(sc, dtype=dtype, **kw) if law == "mujoco" else rb.World(sc, dtype=dtype, law=law)) as w:
        w.step(steps)                                   # warm-up (captures the step graph)
        rates = []
        for _ in range(reps):
            w.set_state(sc.qpos0, sc.qvel0)
            t0 = time.perf_counter()
            w.step(steps)                               # synchronous
            rates.append(steps / (time.perf_counter() - t0))
    return _summary(rates)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="+", default=[1, 1024, 16384, 262144])
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--law", default="mujoco", choices=["mujoco", "balls"],
                    help="balls: scene ball_collision under the two-ball law")
    ap.add_argument("--sampled", type=int, default=0, metavar="EVERY",
                    help="time run_sampled(steps, EVERY) against step(EVERY) + get_state() in a loop")
    ap.add_argument("--per-env", action="store_true",
                    help="also run every E through the per-environment (ENVS) instance, alternating with the plain run")
    ap.add_argument("--incline-sweep", type=int, default=0, metavar="N",
                    help="N cube-incline angles as one batch against N one-environment batches")
    ap.add_argument("--box-pile", default="", metavar="NX,NY,LAYERS",
                    help="scene box_pile(NX, NY, LAYERS), a friction sweep, against one World(max_partners=32)")
    ap.add_argument("--wide-pile", default="", metavar="NX,NY,LAYERS",
                    help="--box-pile for a pile of 65..256 bodies (a wide batch) against one World(max_partners=32)")
    ap.add_argument("--device-loop", type=int, default=0, metavar="K",
                    help="a closed loop's iteration of K steps through device tensors against host arrays")
    ap.add_argument("--sampled-device", type=int, default=0, metavar="EVERY",
                    help="time run_sampled_device(steps, EVERY) against run_sampled(steps, EVERY)")
    ap.add_argument("--contacts", type=int, default=-1, metavar="R",
                    help="time the contact query with R records per body, after --steps settling steps")
    ap.add_argument("--impulses", type=int, default=-1, metavar="R",
                    help="time the impulse query with R records per body, after --steps settling steps")
    ap.add_argument("--sampled-impulses", type=int, default=0, metavar="EVERY",
                    help="time run_sampled_impulses_device(steps, EVERY), all outputs and net alone, against "
                         "run_sampled_device and, at EVERY 1, against impulses_device + step_async per step")
    ap.add_argument("--ragged", default="", metavar="LO,HI",
                    help="an ensemble with body counts spread over LO..HI: one ragged batch against one batch per shape")
    ap.add_argument("--ragged-scene", default="flat_spheres", choices=["flat_spheres", "box_pile"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not a.out:
        a.out = os.path.join(ROOT, "profiles", "batch_ragged", f"ragged_{a.ragged_scene}_{a.ragged.replace(',', '_')}.json") \
            if a.ragged else os.path.join(ROOT, "profiles", "batch", "batch_bench.json")
        if a.impulses >= 0:
            scene = "box_pile_" + a.box_pile.replace(",", "_") if a.box_pile else "multi_sphere4"
            a.out = os.path.join(ROOT, "profiles", "batch_impulses", f"impulses_{scene}_R{a.impulses}.json")
        if a.sampled_impulses:
            scene = "box_pile_" + a.box_pile.replace(",", "_") if a.box_pile else "multi_sphere4"
            a.out = os.path.join(ROOT, "profiles", "batch_sampled_impulses", f"sensed_{scene}_every{a.sampled_impulses}.json")

    import rbhip
    from rbhip import scenes
    rbhip.load()
    sc = scenes.ball_collision() if a.law == "balls" else scenes.multi_sphere4()
    res = dict(bench="batch_bench", scene=sc.name if a.law == "balls" else "multi_sphere4", bodies_per_env=sc.n,
               dtype=a.dtype, steps=a.steps, unit="environment-steps per second",
               version=rbhip.load().rb_version().decode())
    if a.law != "mujoco":
        res["law"] = a.law
    if a.ragged:
        if a.law != "mujoco" or a.dtype != "f64" or a.sampled or a.per_env or a.incline_sweep or a.device_loop or \
                a.sampled_device or a.contacts >= 0 or a.impulses >= 0 or a.box_pile or a.wide_pile:
            raise SystemExit("--ragged: on its own, f64, under the default law")
        lo, hi = (int(t) for t in a.ragged.split(","))
        if not 1 <= lo <= hi <= 256:
            raise SystemExit("--ragged LO,HI: 1 <= LO <= HI <= 256")
        res.update(scene=f"ragged {a.ragged_scene}", bodies_per_env=hi, counts=f"{lo}..{hi}")
        res["ragged"] = {str(E): bench_ragged(rbhip, a.ragged_scene, lo, hi, E, a.steps, a.reps) for E in a.envs}
    elif a.sampled_impulses:
        if a.law != "mujoco" or a.sampled or a.per_env or a.incline_sweep or a.device_loop or a.sampled_device or \
                a.contacts >= 0 or a.impulses >= 0 or a.wide_pile or a.sampled_impulses < 1:
            raise SystemExit("--sampled-impulses EVERY >= 1: on its own (with --box-pile for a mixed template), under the "
                             "default law")
        if a.box_pile:
            sc = scenes.box_pile(*(int(t) for t in a.box_pile.split(",")))
            res.update(scene=sc.name, bodies_per_env=sc.n)
        res.update(unit="seconds per run", every=a.sampled_impulses)
        res["sampled_impulses"] = {str(E): bench_sampled_impulses(rbhip, sc, E, a.steps, a.sampled_impulses, a.reps, a.dtype)
                                   for E in a.envs}
    elif a.impulses >= 0:
        if a.law != "mujoco" or a.sampled or a.per_env or a.incline_sweep or a.device_loop or a.sampled_device or \
                a.contacts >= 0 or a.wide_pile:
            raise SystemExit("--impulses: on its own (with --box-pile for a mixed template), under the default law")
        if a.box_pile:
            sc = scenes.box_pile(*(int(t) for t in a.box_pile.split(",")))
            res.update(scene=sc.name, bodies_per_env=sc.n)
        res.update(unit="seconds per call")
        res["impulses"] = {str(E): bench_impulses(rbhip, sc, E, a.impulses, a.steps, a.reps, a.dtype) for E in a.envs}
    elif a.contacts >= 0:
        if a.law != "mujoco" or a.sampled or a.per_env or a.incline_sweep or a.device_loop or a.sampled_device:
            raise SystemExit("--contacts: on its own (with --box-pile for a mixed template), under the default law")
        if a.box_pile:
            sc = scenes.box_pile(*(int(t) for t in a.box_pile.split(",")))
            res.update(scene=sc.name, bodies_per_env=sc.n)
        res.update(unit="seconds per call")
        res["contacts"] = {str(E): bench_contacts(rbhip, sc, E, a.contacts, a.steps, a.reps, a.dtype) for E in a.envs}
    elif a.box_pile or a.wide_pile:
        if a.law != "mujoco" or a.sampled or a.per_env or a.incline_sweep or (a.box_pile and a.wide_pile):
            raise SystemExit("--box-pile / --wide-pile: one of them, the plain measurement under the default law only")
        sc = scenes.box_pile(*(int(t) for t in (a.box_pile or a.wide_pile).split(",")))
        if a.wide_pile and not 64 < sc.n <= 256:
            raise SystemExit(f"--wide-pile: a pile of 65..256 bodies ({sc.n} given; --box-pile takes up to 64)")
        res.update(scene=sc.name, bodies_per_env=sc.n, sweep="friction 0.2 .. 0.8")
        if a.wide_pile:
            res.update(pile=a.wide_pile, wide=True)
        res["world"] = bench_world(rbhip, sc, a.steps, a.reps, a.dtype, max_partners=32)
        res["batch"] = {str(E): bench_batch(rbhip, sc, E, a.steps, a.reps, a.dtype, sweep={"friction": (0.2, 0.8)})
                        for E in a.envs}
        res["world_after"] = bench_world(rbhip, sc, a.steps, a.reps, a.dtype, max_partners=32)
        w = res["world"]["median"]
        res["ratio_vs_world"] = {E: dict(median=r["median"] / w, min=r["min"] / w, max=r["max"] / w)
                                 for E, r in res["batch"].items()}
    elif a.device_loop or a.sampled_device:
        if a.law != "mujoco" or a.sampled or a.per_env or a.incline_sweep:
            raise SystemExit("--device-loop / --sampled-device: on their own, under the default law")
        if a.device_loop:
            res.update(unit="seconds per iteration", steps_per_iteration=a.device_loop, iterations=a.steps)
            res["device_loop"] = {str(E): bench_device_loop(rbhip, sc, E, a.device_loop, a.steps, a.reps, a.dtype)
                                  for E in a.envs}
        else:
            res.update(unit="seconds per run", every=a.sampled_device)
            res["sampled_device"] = {str(E): bench_sampled_device(rbhip, sc, E, a.steps, a.sampled_device, a.reps, a.dtype)
                                     for E in a.envs}
    elif a.incline_sweep:
        res.update(scene="cube_incline", bodies_per_env=1, dtype="f64", unit="seconds per run")
        res["incline_sweep"] = bench_incline_sweep(rbhip, a.incline_sweep, a.steps, a.reps)
    elif a.sampled:
        res["unit"] = "seconds per run"
        res["every"] = a.sampled
        res["sampled"] = {str(E): bench_sampled(rbhip, sc, E, a.steps, a.sampled, a.reps, a.dtype, a.law) for E in a.envs}
    else:
        res["world"] = bench_world(rbhip, sc, a.steps, a.reps, a.dtype, a.law)
        if a.per_env:
            if a.law != "mujoco":
                raise SystemExit("--per-env: the two-ball law takes no per-environment planes or forces")
            both = {str(E): bench_batch_env(rbhip, sc, E, a.steps, a.reps, a.dtype) for E in a.envs}
            res["batch"] = {E: r[0] for E, r in both.items()}
            res["batch_env"] = {E: r[1] for E, r in both.items()}
            res["batch_env_no_xfrc"] = {E: r[2] for E, r in both.items()}
            res["env_over_plain"] = {E: r[1]["median"] / r[0]["median"] for E, r in both.items()}
            res["env_no_xfrc_over_plain"] = {E: r[2]["median"] / r[0]["median"] for E, r in both.items()}
        else:
            res["batch"] = {str(E): bench_batch(rbhip, sc, E, a.steps, a.reps, a.dtype, a.law) for E in a.envs}
        res["world_after"] = bench_world(rbhip, sc, a.steps, a.reps, a.dtype, a.law)
        w = res["world"]["median"]
        res["ratio_vs_world"] = {E: dict(median=r["median"] / w, min=r["min"] / w, max=r["max"] / w)
                                 for E, r in res["batch"].items()}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
