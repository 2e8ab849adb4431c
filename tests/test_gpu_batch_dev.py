"""The device-resident boundary of a batch on the GPU (BatchWorld.use_stream,
step_async, sync, set_state_device, get_state_device, set_xfrc_device,
status_device, run_sampled_device): torch tensors on the device in and out,
compared word for word, without a tolerance anywhere, with the host path,
with a twin batch, or with the oracle run one environment at a time."""
import ctypes as C

import numpy as np
import pytest

from sweep_scenes import oracle_envs

pytestmark = pytest.mark.gpu

EINVAL, EDOM, EUNSUPPORTED = -22, -33, -95
NP = {"f64": np.float64, "f32": np.float32}


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _same(a, b):
    """Bit identity, as words of the arrays' own width (the sign of zeros and NaN payloads count)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype, (a.dtype, b.dtype)
    w = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
    return a.shape == b.shape and np.array_equal(a.view(w), b.view(w))


def _host(t):
    return t.cpu().numpy()


def _dev(torch, a, offset=False):
    """The array on the device; offset: as a view that starts one element into its allocation."""
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()                # (torch wraps writable arrays only)
    if not offset:
        return torch.from_numpy(a).to("cuda:0")
    flat = torch.empty(a.size + 1, dtype=torch.from_numpy(a).dtype, device="cuda:0")
    view = flat[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def _jittered(sc, E, seed=3):
    """The scene's start state per environment, xy moved by +-0.02 and velocities by N(0, 0.3)."""
    rng = np.random.default_rng(seed)
    q = np.broadcast_to(sc.qpos0, (E, sc.n, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (E, sc.n, 6)).copy()
    q[:, :, :2] += rng.uniform(-0.02, 0.02, (E, sc.n, 2))
    v += rng.normal(0.0, 0.3, (E, sc.n, 6))
    return q, v


def _forces(E, M, n, seed):
    """n seeded applied-force arrays (E, M, 6): force N(0, 0.5), torque N(0, 0.05)."""
    rng = np.random.default_rng(seed)
    return [np.concatenate([rng.normal(0.0, 0.5, (E, M, 3)), rng.normal(0.0, 0.05, (E, M, 3))], axis=2)
            for _ in range(n)]


def _batch(rb, torch, sc, E, q=None, v=None, restitution=None, **kw):
    """A batch on torch's current stream (the documented way to share tensors with torch)."""
    b = rb.BatchWorld(sc, E, **kw)
    if restitution is not None:
        b.set_params(restitution=restitution)
    if q is not None:
        b.set_state(q, v)
    b.use_stream(torch.cuda.current_stream().cuda_stream)
    return b


# ------------------------------------------------------------------ 1. round trip
def _round_trip(rb, torch, sc, E, batch_dtype, io, offset):
    q, v = _jittered(sc, E)
    q[:, :, 3:] += 0.125                                    # (every column carries its own values)
    qi, vi = q.astype(NP[io]), v.astype(NP[io])
    with _batch(rb, torch, sc, E, dtype=batch_dtype) as b:
        b.set_state_device(_dev(torch, qi, offset), _dev(torch, vi, offset))
        hq, hv = b.get_state()                             # the host path: the uploaded words, as the batch holds them
        assert _same(hq, qi.astype(NP[batch_dtype]).astype(np.float64))
        assert _same(hv, vi.astype(NP[batch_dtype]).astype(np.float64))
        oq = _dev(torch, np.zeros((E, sc.n, 7), NP[io]), offset)
        ov = _dev(torch, np.zeros((E, sc.n, 6), NP[io]), offset)
        rq, rv = b.get_state_device(oq, ov)
        assert rq is oq and rv is ov
        assert _same(_host(oq), hq.astype(NP[io])) and _same(_host(ov), hv.astype(NP[io]))
        # omitted outputs: new tensors of the asked type (None: the batch's)
        nq, nv = b.get_state_device(dtype=io)
        assert _same(_host(nq), hq.astype(NP[io])) and _same(_host(nv), hv.astype(NP[io]))
        dq, _ = b.get_state_device()
        assert _same(_host(dq), hq.astype(NP[batch_dtype]))
        assert b.sync() == 0


@pytest.mark.parametrize("batch_dtype", ["f64", "f32"])
@pytest.mark.parametrize("io", ["f64", "f32"])
def test_round_trip(rb, torch, batch_dtype, io):
    """E = 17 environments of four balls (four per wave, ragged; 68 rows: one
    short span), every element type against every real type; a narrowing get
    equals the host's float64 rows cast to float32."""
    from rbhip import scenes
    _round_trip(rb, torch, scenes.multi_sphere4(), 17, batch_dtype, io, False)


@pytest.mark.parametrize("io", ["f64", "f32"])
def test_round_trip_unaligned_views(rb, torch, io):
    """Every tensor a view one element into its allocation: the element-wide path."""
    from rbhip import scenes
    _round_trip(rb, torch, scenes.multi_sphere4(), 17, "f64", io, True)


@pytest.mark.parametrize("which", ["M63", "M1"])
def test_round_trip_other_sizes(rb, torch, which):
    """M = 63 (E = 3: environments that straddle spans) and M = 1 (E = 130: a
    span of 130 environments), aligned and not."""
    from rbhip import scenes
    sc, E = (scenes.balls_pile(9, 7), 3) if which == "M63" else (scenes.single_cube(), 130)
    assert sc.n == (63 if which == "M63" else 1)
    _round_trip(rb, torch, sc, E, "f64", "f64", False)
    _round_trip(rb, torch, sc, E, "f64", "f32", True)


def test_round_trip_several_spans(rb, torch):
    """More than one block: 300 environments of four balls are 1,200 rows, five spans, the last one short."""
    from rbhip import scenes
    _round_trip(rb, torch, scenes.multi_sphere4(), 300, "f64", "f64", False)
    _round_trip(rb, torch, scenes.multi_sphere4(), 300, "f32", "f64", True)


# ------------------------------------------------------------------ 2. masked reset
def test_masked_reset(rb, torch):
    from rbhip import scenes
    sc, E = scenes.multi_sphere4(), 17
    q0, v0 = _jittered(sc, E)
    q0[5, 2, 2] = np.nan                                    # environment 5 fails at its first step
    qn, vn = _jittered(sc, E, seed=11)
    with _batch(rb, torch, sc, E, q0, v0) as b:
        assert b.step(50) == 1
        bq, bv = b.get_state()
        masked = [0, 3, 16]
        others = [k for k in range(E) if k not in masked]
        up_q, up_v = np.full_like(qn, np.nan), np.full_like(vn, np.nan)
        up_q[masked], up_v[masked] = qn[masked], vn[masked]
        mask = np.zeros(E, bool)
        mask[masked] = True
        b.set_state_device(_dev(torch, up_q), _dev(torch, up_v), mask=_dev(torch, mask))
        code, done = b.status_device()
        code, done = _host(code), _host(done)
        assert code.dtype == np.int32 and done.dtype == np.int64
        gq, gv = b.get_state()
        assert _same(gq[others], bq[others]) and _same(gv[others], bv[others])
        assert _same(gq[masked], qn[masked]) and _same(gv[masked], vn[masked])
        assert (done[masked] == 0).all() and done[5] == 0
        assert (done[[k for k in others if k != 5]] == 50).all()
        assert code[5] == EDOM and not code[[k for k in range(E) if k != 5]].any()     # not masked: still failed
        hc, hd = b.status()
        assert np.array_equal(hc, code) and np.array_equal(hd, done)
        # a uint8 mask on environment 5 alone clears it; the unaligned path
        mask5 = np.zeros(E, np.uint8)
        mask5[5] = 7
        up_q[:], up_v[:] = np.nan, np.nan
        up_q[5], up_v[5] = qn[5], vn[5]
        b.set_state_device(_dev(torch, up_q, True), _dev(torch, up_v, True), mask=_dev(torch, mask5, True))
        code, done = (_host(t) for t in b.status_device())
        assert not code.any() and done[5] == 0 and (done[[1, 2, 4, 6]] == 50).all()
        g2q, g2v = b.get_state()
        keep = [k for k in range(E) if k != 5]
        assert _same(g2q[keep], gq[keep]) and _same(g2v[keep], gv[keep])
        assert _same(g2q[5], qn[5]) and _same(g2v[5], vn[5])
        b.step_async(3)
        assert b.sync() == 0
        assert (_host(b.status_device()[1])[[0, 1, 5]] == [3, 53, 3]).all()
        # float32 tensors (four elements per 16-byte access, across the mask's edges), neighbours masked
        s3q, s3v = b.get_state()
        masked = [1, 2, 9, 16]
        keep = [k for k in range(E) if k not in masked]
        up_q, up_v = np.full(qn.shape, np.nan, np.float32), np.full(vn.shape, np.nan, np.float32)
        up_q[masked], up_v[masked] = qn[masked], vn[masked]
        mask = np.zeros(E, bool)
        mask[masked] = True
        b.set_state_device(_dev(torch, up_q), _dev(torch, up_v), mask=_dev(torch, mask))
        g3q, g3v = b.get_state()
        assert _same(g3q[keep], s3q[keep]) and _same(g3v[keep], s3v[keep])
        assert _same(g3q[masked], up_q[masked].astype(np.float64)) and _same(g3v[masked], up_v[masked].astype(np.float64))
        assert (_host(b.status_device()[1])[[0, 1, 2, 5, 9, 16]] == [3, 0, 0, 3, 0, 0]).all()


# ------------------------------------------ 3. async steps against the oracle, forces that change
SEGMENTS, SEG_STEPS = 30, 8


def _forced_inputs(sc, E, segments, seed):
    q0, v0 = _jittered(sc, E)
    return dict(sc=sc, E=E, q0=q0, v0=v0, xf=_forces(E, sc.n, segments, seed))


def _forced_reference(oracle, d, scs, max_partners=16):
    q, v = d["q0"], d["v0"]
    plane = np.zeros(d["E"], np.int64)
    for xf in d["xf"]:
        q, v, _, st = oracle_envs(oracle, scs, q, v, SEG_STEPS, xfrc=xf, max_partners=max_partners)
        plane += st["plane"]
    for a in (q, v, plane, d["q0"], d["v0"], *d["xf"]):
        a.setflags(write=False)
    return dict(d, q=q, v=v, plane=plane)


def _forced_loop(torch, b, d):
    """Every segment: new forces, SEG_STEPS steps; no synchronisation in between."""
    held = []
    for xf in d["xf"]:
        t = _dev(torch, xf)
        held.append(t)
        b.set_xfrc_device(t)
        b.step_async(SEG_STEPS)
    return held


RESTITUTION5 = np.linspace(0.3, 0.8, 5)


@pytest.fixture(scope="module")
def forced4(oracle):
    from rbhip import scenes
    sc = scenes.multi_sphere4()
    d = _forced_inputs(sc, 5, SEGMENTS, seed=5)
    scs = [sc.with_(restitution=float(e)) for e in RESTITUTION5]
    return _forced_reference(oracle, d, scs)


def test_async_steps_with_changing_forces_match_the_oracle(rb, torch, forced4):
    d = forced4
    assert (d["plane"] >= 5).all(), d["plane"]             # every environment bounced under the forces
    assert len({d["q"][k].tobytes() for k in range(d["E"])}) == d["E"]
    with _batch(rb, torch, d["sc"], d["E"], d["q0"], d["v0"], restitution=RESTITUTION5) as b:
        held = _forced_loop(torch, b, d)
        assert b.sync() == 0
        gq, gv = b.get_state_device()
        assert _same(_host(gq), d["q"]) and _same(_host(gv), d["v"])
        assert (_host(b.status_device()[1]) == SEGMENTS * SEG_STEPS).all()
        del held


# ------------------------------------------------------------------ 4. the same loop on a box pile
def test_async_steps_on_a_box_pile_match_the_oracle(rb, torch, oracle):
    from rbhip import scenes
    sc = scenes.box_pile(1, 1, 3, seed=1)
    d = _forced_inputs(sc, 5, 15, seed=6)                   # 120 steps
    d = _forced_reference(oracle, d, [sc] * 5, max_partners=32)
    assert (d["plane"] >= 20).all(), d["plane"]
    assert len({d["q"][k].tobytes() for k in range(5)}) == 5
    with _batch(rb, torch, sc, 5, d["q0"], d["v0"]) as b:
        held = _forced_loop(torch, b, d)
        assert b.sync() == 0
        gq, gv = b.get_state_device()
        assert _same(_host(gq), d["q"]) and _same(_host(gv), d["v"])
        del held


# ------------------------------------------------------------------ 5. closed loop, device against host
def test_closed_loop_device_against_host(rb, torch):
    from rbhip import scenes
    sc, E = scenes.multi_sphere4(), 5
    q0, v0 = _jittered(sc, E)
    with _batch(rb, torch, sc, E, q0, v0, restitution=RESTITUTION5) as a, \
            _batch(rb, torch, sc, E, q0, v0, restitution=RESTITUTION5) as h:
        for it in range(25):
            q, v = a.get_state_device()
            f = torch.cat([0.3 * torch.sin(3.0 * q[..., :3]) - 0.4 * v[..., :3], -0.02 * v[..., 3:]], dim=-1).contiguous()
            a.set_xfrc_device(f)
            a.step_async(4)
            h.set_xfrc(_host(f))
            h.step(4)
            aq, av = a.get_state_device()
            hq, hv = h.get_state()
            assert _same(_host(aq), hq) and _same(_host(av), hv), it
        assert a.sync() == 0
        assert not _same(hq, q0)


# ------------------------------------------------------------------ 6. sampled to the device
def _sampled_pair(rb, torch, q0, v0, **kw):
    from rbhip import scenes
    sc = scenes.multi_sphere4()
    return (_batch(rb, torch, sc, 5, q0, v0, restitution=RESTITUTION5, **kw),
            _batch(rb, torch, sc, 5, q0, v0, restitution=RESTITUTION5, **kw))


@pytest.mark.parametrize("velocities", [True, False])
@pytest.mark.parametrize("buffer", ["default", "three_samples"])
def test_sampled_to_the_device(rb, torch, velocities, buffer, monkeypatch):
    """600 steps sampled every 7th (sample 36 is step 259, inside the second
    launch), against the host path on a twin batch; with a buffer of exactly
    three samples of the device path's size, 29 drains without a sync."""
    from rbhip import scenes
    sc = scenes.multi_sphere4()
    q0, v0 = _jittered(sc, 5)
    if buffer == "three_samples":
        monkeypatch.setenv("RBHIP_BATCH_SAMPLE_BYTES", str(3 * 5 * sc.n * (13 if velocities else 7) * 8))
    a, h = _sampled_pair(rb, torch, q0, v0)
    with a, h:
        dq, dv = a.run_sampled_device(600, 7, velocities=velocities)
        hq, hv, nf = h.run_sampled(600, 7, velocities=velocities)
        assert a.sync() == 0 and nf == 0
        assert tuple(dq.shape) == (85, 5, 4, 7) and _same(_host(dq), hq)
        assert not _same(hq[35], hq[36])
        if velocities:
            assert _same(_host(dv), hv)
        else:
            assert dv is None and hv is None
        for x, y in zip(a.get_state(), h.get_state()):
            assert _same(x, y)
        assert np.array_equal(a.status()[1], h.status()[1]) and (a.status()[1] == 600).all()
        # into float32 tensors of the caller, unaligned
        a.set_state(q0, v0)
        oq = _dev(torch, np.zeros((85, 5, 4, 7), np.float32), True)
        ov = _dev(torch, np.zeros((85, 5, 4, 6), np.float32), True) if velocities else None
        a.run_sampled_device(600, 7, velocities=velocities, out_qpos=oq, out_qvel=ov)
        assert _same(_host(oq), hq.astype(np.float32))
        if velocities:
            assert _same(_host(ov), hv.astype(np.float32))
        assert a.sync() == 0


def test_sampled_to_the_device_edges(rb, torch, monkeypatch):
    from rbhip import scenes
    sc = scenes.multi_sphere4()
    q0, v0 = _jittered(sc, 5)
    q0[2, 1, 0] = np.nan                                    # environment 2 fails at once
    a, h = _sampled_pair(rb, torch, q0, v0)
    with a, h:
        # a failing environment's rows repeat its frozen state
        dq, dv = a.run_sampled_device(40, 7)
        hq, hv, nf = h.run_sampled(40, 7)
        assert a.sync() == 1 and nf == 1
        assert _same(_host(dq), hq) and _same(_host(dv), hv)
        for s in range(5):
            assert _same(_host(dq)[s, 2], q0[2]) and _same(_host(dv)[s, 2], v0[2])
        # every > nsteps: no sample, the run is still stepped
        dq, dv = a.run_sampled_device(5, 7)
        assert tuple(dq.shape) == (0, 5, 4, 7) and tuple(dv.shape) == (0, 5, 4, 6)
        assert a.sync() == 1
        assert (np.delete(a.status()[1], 2) == 45).all() and a.status()[1][2] == 0
    # a bound one byte below one sample: refused, nothing stepped
    q0[2, 1, 0] = 0.0
    monkeypatch.setenv("RBHIP_BATCH_SAMPLE_BYTES", str(5 * sc.n * 13 * 8 - 1))
    with _batch(rb, torch, sc, 5, q0, v0) as b:
        with pytest.raises(rb.RbError) as exc:
            b.run_sampled_device(40, 7)
        assert exc.value.code == EINVAL
        assert b.sync() == 0 and (b.status()[1] == 0).all()
        assert _same(b.get_state()[0], q0)
        b.run_sampled_device(40, 7, velocities=False)       # (7 rows fit)
        assert b.sync() == 0 and (b.status()[1] == 40).all()


# ------------------------------------------------------------------ 7. refusals
def test_non_finite_force_is_refused_on_the_device(rb, torch):
    from rbhip import scenes
    sc, E = scenes.multi_sphere4(), 5
    q0, v0 = _jittered(sc, E)
    good, bad = _forces(E, sc.n, 2, seed=9)
    bad[2, 1, 4] = np.nan
    bad[3, 0, 0] = np.inf                                   # (a later slot: the smallest one is named)
    with _batch(rb, torch, sc, E, q0, v0) as a, _batch(rb, torch, sc, E, q0, v0) as twin:
        for b in (a, twin):
            b.set_xfrc_device(_dev(torch, good))
            b.step_async(8)
            assert b.sync() == 0
        a.set_xfrc_device(_dev(torch, bad))                 # returns: the host cannot know
        with pytest.raises(rb.RbError, match="environment 2, body 1") as exc:
            a.sync()
        assert exc.value.code == EINVAL
        assert a.sync() == 0                                # reported once
        for b in (a, twin):
            b.step_async(8)
            assert b.sync() == 0
        for x, y in zip(a.get_state(), twin.get_state()):
            assert _same(x, y)                              # the rows kept the earlier, valid forces
        # float32 forces: the same check
        a.set_xfrc_device(_dev(torch, bad.astype(np.float32), True))
        with pytest.raises(rb.RbError, match="environment 2, body 1"):
            a.sync()
        assert a.sync() == 0


def test_host_pointers_are_refused(rb, torch):
    from rbhip import scenes, _lib
    sc, E = scenes.multi_sphere4(), 5
    q0, v0 = _jittered(sc, E)
    hq, hv = np.zeros((2, E, sc.n, 7)), np.zeros((2, E, sc.n, 6))
    code, done, mask = np.zeros(E, np.int32), np.zeros(E, np.int64), np.ones(E, np.uint8)
    dq, dv = _dev(torch, q0), _dev(torch, v0)
    P, D = _lib.ptr, lambda t: C.c_void_p(t.data_ptr())
    with _batch(rb, torch, sc, E, q0, v0) as b:
        L, h, p = b._L, b._h, b._params(None, None, None, None)
        calls = [lambda: L.rb_batch_set_state_dev(h, None, P(hq), D(dv), 0),
                 lambda: L.rb_batch_set_state_dev(h, None, D(dq), P(hv), 0),
                 lambda: L.rb_batch_set_state_dev(h, P(mask), D(dq), D(dv), 0),
                 lambda: L.rb_batch_get_state_dev(h, P(hq), None, 0),
                 lambda: L.rb_batch_get_state_dev(h, D(dq), P(hv), 0),
                 lambda: L.rb_batch_set_xfrc_dev(h, P(hv), 0),
                 lambda: L.rb_batch_status_dev(h, P(code), None),
                 lambda: L.rb_batch_status_dev(h, None, P(done)),
                 lambda: L.rb_batch_run_sampled_dev(h, 2, 1, *p, P(hq), None, 0),
                 lambda: L.rb_batch_run_sampled_dev(h, 2, 1, *p, D(_dev(torch, hq)), P(hv), 0)]
        for k, call in enumerate(calls):
            assert call() == EINVAL, k
            assert b"not device memory" in L.rb_last_error(), k
            assert b.sync() == 0, k                         # nothing was enqueued, no HIP error is left behind
        torch.cuda.synchronize()
        assert (b.status()[1] == 0).all()
        for x, y in zip(b.get_state(), (q0, v0)):
            assert _same(x, y)
        assert b.step(1) == 0                               # still the plain instances: no forces were set


def test_device_forces_are_unsupported_under_the_two_ball_law(rb, torch):
    from rbhip import scenes
    sc = scenes.ball_collision()
    with _batch(rb, torch, sc, 3, law="balls") as b:
        with pytest.raises(rb.RbError) as exc:
            b.set_xfrc_device(_dev(torch, np.zeros((3, sc.n, 6))))
        assert exc.value.code == EUNSUPPORTED
        assert b.sync() == 0


# ------------------------------------------------------------------ 8. the caller's stream
def test_callers_stream(rb, torch, forced4):
    d = forced4
    s = torch.cuda.Stream()
    b = rb.BatchWorld(d["sc"], d["E"])
    try:
        b.set_params(restitution=RESTITUTION5)
        b.set_state(d["q0"], d["v0"])
        b.use_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            held = _forced_loop(torch, b, d)
            gq, gv = b.get_state_device()
            got = _host(gq), _host(gv)                      # (torch waits for s, not the batch)
        assert _same(got[0], d["q"]) and _same(got[1], d["v"])
        assert b.sync() == 0
        # back on the null stream: the same run again
        b.use_stream(None)
        b.set_state(d["q0"], d["v0"])
        held += _forced_loop(torch, b, d)
        gq, gv = b.get_state_device()
        torch.cuda.synchronize()
        assert _same(_host(gq), d["q"]) and _same(_host(gv), d["v"])
        b.use_stream(s.cuda_stream)
    finally:
        b.close()
    # the stream is the caller's: it outlives the batch
    with torch.cuda.stream(s):
        x = torch.arange(1000, device="cuda:0", dtype=torch.float64) * 2.0
    s.synchronize()
    assert float(x.sum().item()) == 999000.0
    del held
