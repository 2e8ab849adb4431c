"""Contact-impulse curves recorded inside a sampled run
(rb_batch_run_sampled_impulses, rb_batch_run_sampled_impulses_dev;
BatchWorld.run_sampled_impulses / run_sampled_impulses_device; kernels in
rb_batch_sensed.hip).

1. State: qpos, qvel, the final state, status and n_failed equal run_sampled's
   of a twin batch in every word.
2. Net, against the query: a Python loop on a third twin, per step
   impulses(max_records=0).net, step(1), status(); a row joins its window's sum
   only if the environment is still healthy after the step; sums in the real
   type from +0; words compared, every in {1, 3}.
3. Cuts: windows that straddle the 256-step launches, a window over three
   launches, drains in mid-run, each against the same run made call by call.
4. Failure.  5. The device form, the net-only call.  6. Refusals.

Shapes are those of tests/test_gpu_batch_impulses.py: M = 1, 4 (one wave, idle
lanes at E = 7), 70 (128 threads, boxes), 144 (192 threads), a population of
1..8 bodies, a population of M = 1; E between 2 and 24."""
import numpy as np
import pytest

import impulse_model as IM

pytestmark = pytest.mark.gpu

EINVAL = -22
EDOM = -33
EUNSUPPORTED = -95


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _same(a, b, dtype="f64"):
    """Word for word (the sign of zeros counts), as reals of the batch's type."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(IM.words(a, dtype), IM.words(b, dtype))


def box_sweep():
    from rbhip import scenes
    return [scenes.box_pile(1, 1, 3).with_(friction=f) for f in (0.0, 0.2, 0.5, 0.8, 1.2)]


def sphere_sweep(n=7):
    from rbhip import scenes
    return [scenes.multi_sphere4().with_(restitution=float(e)) for e in np.linspace(0.2, 0.95, 7)][:n]


def ragged_scenes():
    from rbhip import scenes
    return [scenes.box_pile(1 + (s // 3) % 2, 1, 1 + s % 3, seed=s, sphere_every=(0, 1, 3)[(s // 6) % 3])
            for s in range(24)]


def _make_case(rb, name, dtype="f64"):
    """(batch, present (E, M) bool, steps to run before the recorded run)"""
    from rbhip import scenes
    if name == "single_cube":                            # M = 1: the one-box path of the sphere instance
        scs = [scenes.single_cube().with_(friction=f) for f in (0.1, 0.5, 0.9)]
        return rb.BatchWorld.from_scenes(scs, dtype=dtype), np.ones((3, 1), bool), 0
    if name == "multi_sphere4":                          # E = 7: idle lanes in the last wave; first impact at step 62
        return rb.BatchWorld.from_scenes(sphere_sweep(), dtype=dtype), np.ones((7, 4), bool), 62
    if name == "box_pile_1_1_3":                         # mixed, one wave
        return rb.BatchWorld.from_scenes(box_sweep(), dtype=dtype), np.ones((5, 4), bool), 0
    if name == "box_pile_4_4_4":                         # 70 bodies: 128 threads, boxes
        b = rb.BatchWorld(scenes.box_pile(4, 4, 4), 2, dtype=dtype)
        b.set_params(friction=[0.2, 0.9])
        return b, np.ones((2, 70), bool), 0
    if name == "flat_spheres_12_12":                     # 144 bodies: 192 threads, spheres
        b = rb.BatchWorld(scenes.flat_spheres(12, 12, spacing=0.19), 2, dtype=dtype)
        b.set_params(restitution=[0.3, 0.8])
        return b, np.ones((2, 144), bool), 0
    if name == "population":
        scs = ragged_scenes()
        n = np.array([sc.n for sc in scs])
        assert sorted(set(n)) == list(range(1, 9)) and n.sum() == 87
        return rb.BatchWorld.from_ragged_scenes(scs, dtype=dtype), np.arange(8)[None, :] < n[:, None], 0
    if name == "population_of_one":                      # M = 1 with kinds per environment: the box instance at M = 1
        cube = scenes.single_cube()
        scs = [cube, scenes.single_sphere().with_(dt=cube.dt, threshold=cube.threshold)] * 3
        return rb.BatchWorld.from_ragged_scenes(scs, dtype=dtype), np.ones((6, 1), bool), 0
    assert name == "planes_gravity_forces"
    scs = box_sweep()
    E, M = len(scs), scs[0].n
    b = rb.BatchWorld.from_scenes(scs, dtype=dtype)
    rng = np.random.default_rng(5)
    planes = np.tile(np.asarray(scs[0].planes, np.float64), (E, 1, 1))
    planes[:, :, 0] += np.linspace(-0.05, 0.05, E)[:, None]              # tilted floors
    planes[:, :, :3] /= np.linalg.norm(planes[:, :, :3], axis=2, keepdims=True)
    gravity = np.tile(np.asarray(scs[0].gravity, np.float64), (E, 1))
    gravity[:, 1] = np.linspace(-1.0, 1.0, E)
    xfrc = rng.uniform(-0.5, 0.5, (E, M, 6))
    xfrc[1, 2] = 0.0                                                    # one all-zero force row among them
    b.set_planes(planes)
    b.set_gravity(gravity)
    b.set_xfrc(xfrc)
    return b, np.ones((E, M), bool), 0


CASES = [("single_cube", "f64"), ("multi_sphere4", "f64"), ("box_pile_1_1_3", "f64"), ("box_pile_4_4_4", "f64"),
         ("flat_spheres_12_12", "f64"), ("population", "f64"), ("population_of_one", "f64"),
         ("planes_gravity_forces", "f64"), ("multi_sphere4", "f32"), ("box_pile_1_1_3", "f32"), ("population", "f32")]
NSTEPS = 60


def model_steps(b, nsteps):
    """The model's per-step rows on batch b, which it steps: (net (nsteps, E, M, 6)
    of the query before each step, ok (nsteps, E): the environment is still
    healthy after the step, so the step was committed)."""
    nets, oks = [], []
    for _ in range(nsteps):
        nets.append(b.impulses(max_records=0).net)
        b.step(1)
        oks.append(b.status()[0] == 0)
    return np.stack(nets), np.stack(oks)


def model_windows(nets, oks, every, dtype):
    """The windows' sums: committed steps' rows added in step order from +0 in the real type."""
    real = np.float64 if dtype == "f64" else np.float32
    S = nets.shape[0] // every
    out = np.zeros((S,) + nets.shape[1:], real)
    for s in range(S):
        for t in range(s * every, (s + 1) * every):
            out[s] = np.where(oks[t][:, None, None], out[s] + nets[t].astype(real), out[s])
    return out.astype(np.float64)


@pytest.fixture(scope="module")
def reference(rb):
    """Per case, computed once and never changed: run_sampled's answers on one twin
    and the model's per-step rows on another."""
    cache = {}

    def get(name, dtype):
        if (name, dtype) not in cache:
            a, present, pre = _make_case(rb, name, dtype)
            with a:
                assert a.step(pre) == 0
                q, v, nf = a.run_sampled(NSTEPS, 3)
                final = a.get_state()
                status = a.status()
            m, _, _ = _make_case(rb, name, dtype)
            with m:
                assert m.step(pre) == 0
                nets, oks = model_steps(m, NSTEPS)
            cache[name, dtype] = dict(q=q, v=v, nf=nf, final=final, status=status, nets=nets, oks=oks, present=present)
        return cache[name, dtype]
    return get


# ------------------------------------------------------------ 1, 2. state and net
@pytest.mark.parametrize("name,dtype", CASES)
def test_state_is_run_sampleds_and_net_is_the_querys(rb, reference, name, dtype):
    ref = reference(name, dtype)
    present = ref["present"]
    for every in (3, 1):
        b, _, pre = _make_case(rb, name, dtype)
        with b:
            assert b.step(pre) == 0
            q, v, net, nf = b.run_sampled_impulses(NSTEPS, every)
            final, status = b.get_state(), b.status()
        # ---- 1. the state, against run_sampled of the twin ----
        if every == 3:
            assert _same(q, ref["q"]) and _same(v, ref["v"]) and nf == ref["nf"]
        else:
            assert _same(q[2::3], ref["q"]) and _same(v[2::3], ref["v"]) and nf == ref["nf"]
        assert _same(final[0], ref["final"][0]) and _same(final[1], ref["final"][1])
        assert np.array_equal(status[0], ref["status"][0]) and np.array_equal(status[1], ref["status"][1])
        # ---- 2. the net rows, against the query ----
        want = model_windows(ref["nets"], ref["oks"], every, dtype)
        hit = (ref["nets"] != 0).any(axis=3)                        # (step, env, body): a nonzero row of the query
        S = NSTEPS // every
        per_window = hit[:S * every].reshape(S, every, *hit.shape[1:]).sum(axis=1)
        print(f"{name} {dtype} every={every}: {int(hit.sum())} nonzero step rows, {int((per_window >= 2).sum())} windows of "
              f"two or more, {int((per_window == 0).sum())} windows without contact, max |net| {np.abs(net).max():.6g}")
        assert net.shape == (S,) + present.shape + (6,)
        assert (want != 0).any() and (net != 0).any()                # not vacuous
        if every == 3:
            assert (per_window >= 2).any()                          # some window sums two or more steps
        assert _same(net, want, dtype)
        # a body without contact in a window, an absent body: +0 in every word
        quiet = per_window == 0
        assert not IM.words(net, dtype)[quiet].any()
        assert not IM.words(net, dtype)[:, ~present].any()
        if name in ("multi_sphere4", "population"):
            assert quiet.any()


def test_some_body_without_contact_has_a_row_of_plus_zero(rb, reference):
    """(the bouncing spheres are in flight in most windows)"""
    ref = reference("multi_sphere4", "f64")
    hit = (ref["nets"] != 0).any(axis=3)
    assert (~hit).any() and hit.any()


# ------------------------------------------------------------ 3. cuts
def _spheres(rb, dtype="f64"):
    b = rb.BatchWorld.from_scenes(sphere_sweep(5), dtype=dtype)
    assert b.step(62) == 0
    return b


def call_by_call(b, nsteps, every):
    """The run as calls of `every` steps, one window each, and the steps after the last sample."""
    qs, vs, ns = [], [], []
    for _ in range(nsteps // every):
        q, v, n, _ = b.run_sampled_impulses(every, every)
        qs.append(q[0]); vs.append(v[0]); ns.append(n[0])
    b.step(nsteps % every)
    return np.stack(qs), np.stack(vs), np.stack(ns)


@pytest.mark.parametrize("nsteps,every", [(600, 7), (650, 300)])
def test_windows_across_launches(rb, nsteps, every):
    with _spheres(rb) as a, _spheres(rb) as c:
        q, v, net, nf = a.run_sampled_impulses(nsteps, every)
        cq, cv, cn = call_by_call(c, nsteps, every)
        assert nf == 0 and net.shape == (nsteps // every, 5, 4, 6) and (net != 0).any()
        assert _same(q, cq) and _same(v, cv) and _same(net, cn)
        fa, fc = a.get_state(), c.get_state()
        assert _same(fa[0], fc[0]) and _same(fa[1], fc[1])
        assert np.array_equal(a.status()[1], c.status()[1]) and (a.status()[1] == 62 + nsteps).all()
    if every == 7:
        with _spheres(rb) as m:
            nets, oks = model_steps(m, nsteps)
        assert _same(net, model_windows(nets, oks, every, "f64"))


def test_drains_in_mid_run(rb, monkeypatch):
    """The sample buffer (RBHIP_BATCH_SAMPLE_BYTES, read at creation) sized for two
    samples of the host form: 20 samples drain ten times."""
    per = 5 * 4 * 19 * (8 + 8)
    with _spheres(rb) as c:
        cq, cv, cn = call_by_call(c, 60, 3)
    monkeypatch.setenv("RBHIP_BATCH_SAMPLE_BYTES", str(2 * per))
    with _spheres(rb) as a:
        q, v, net, _ = a.run_sampled_impulses(60, 3)
    assert (net != 0).any()
    assert _same(q, cq) and _same(v, cv) and _same(net, cn)
    monkeypatch.setenv("RBHIP_BATCH_SAMPLE_BYTES", str(per - 1))
    with _spheres(rb) as a:
        before = a.status()[1].copy()
        with pytest.raises(rb.RbError) as ei:
            a.run_sampled_impulses(60, 3)
        assert ei.value.code == EINVAL and "RBHIP_BATCH_SAMPLE_BYTES" in str(ei.value)
        assert np.array_equal(a.status()[1], before)
        # the net-only call takes 6 rows a sample: it fits
        _, _, n6, _ = a.run_sampled_impulses(60, 3, positions=False, velocities=False)
    assert _same(n6, cn)


# ------------------------------------------------------------ 4. failure
def _poisoned(rb, poison):
    b = rb.BatchWorld.from_scenes(box_sweep())
    if poison:
        q, v = b.get_state()
        q[0, 1, 0] = np.nan                              # environment 0 fails in its first step
        v[2, 3, 0] = 1.0e8 / b.scene.dt                  # environment 2's sphere leaves the range within some steps
        b.set_state(q, v)
    return b


def test_a_failing_environment_keeps_its_committed_steps(rb):
    nsteps = 84
    with _poisoned(rb, True) as m:
        nets, oks = model_steps(m, nsteps)
        done = m.status()[1]
    f = int(done[2])
    assert done[0] == 0 and 0 < f < nsteps - 14, done
    every = next(e for e in (7, 4, 5) if f % e)          # the failing step lies inside a window that holds committed steps
    with _poisoned(rb, True) as a, _poisoned(rb, True) as r, _poisoned(rb, False) as clean:
        q, v, net, nf = a.run_sampled_impulses(nsteps, every)
        rq, rv, rnf = r.run_sampled(nsteps, every)
        cq, cv, cnet, cnf = clean.run_sampled_impulses(nsteps, every)
        assert nf == rnf == 2 and cnf == 0
        assert _same(q, rq) and _same(v, rv)                                     # frozen rows as run_sampled's
        assert np.array_equal(a.status()[0], [EDOM, 0, EDOM, 0, 0]) and np.array_equal(a.status()[1], r.status()[1])
        assert a.status()[1][2] == f
    want = model_windows(nets, oks, every, "f64")
    assert _same(net, want)
    wf = f // every                                       # the window that holds the failure
    assert (net[wf, 2] != 0).any()                        # the sum of its committed steps
    assert not IM.words(net)[wf + 1:, 2].any() and not IM.words(net)[:, 0].any()   # later windows: +0
    others = [1, 3, 4]
    assert _same(net[:, others], cnet[:, others]) and _same(q[:, others], cq[:, others]) and _same(v[:, others], cv[:, others])


def test_a_failing_body_in_the_second_wave_freezes_the_environment(rb):
    def make(poison):
        b, _, _ = _make_case(rb, "box_pile_4_4_4")
        if poison:
            q, v = b.get_state()
            q[1, 66, 2] = np.nan
            b.set_state(q, v)
        return b
    with make(True) as a, make(True) as r, make(False) as clean:
        q0 = a.get_state()
        q, v, net, nf = a.run_sampled_impulses(12, 3)
        rq, rv, rnf = r.run_sampled(12, 3)
        cq, cv, cnet, _ = clean.run_sampled_impulses(12, 3)
        assert nf == rnf == 1 and np.array_equal(a.status()[1], [12, 0])
        assert _same(q, rq) and _same(v, rv) and _same(a.get_state()[0][1], q0[0][1])
        assert not IM.words(net)[:, 1].any() and (net[:, 0] != 0).any()
        assert _same(net[:, 0], cnet[:, 0]) and _same(q[:, 0], cq[:, 0])


# ------------------------------------------------------------ 5. forms
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_device_form_and_net_only(rb, torch, dtype):
    def make():
        b = rb.BatchWorld.from_scenes(box_sweep(), dtype=dtype)
        return b
    with make() as h, make() as d, make() as d32, make() as n:
        q, v, net, _ = h.run_sampled_impulses(30, 3)
        dq, dv, dn = d.run_sampled_impulses_device(30, 3, dtype="f64")
        assert d.sync() == 0
        assert dq.dtype == torch.float64 and dn.shape == (10, 5, 4, 6)
        assert _same(dq.cpu().numpy(), q) and _same(dv.cpu().numpy(), v) and _same(dn.cpu().numpy(), net)
        out = torch.full((10, 5, 4, 6), float("nan"), dtype=torch.float32, device="cuda")
        fq, fv, fn = d32.run_sampled_impulses_device(30, 3, velocities=False, out_net=out)
        assert d32.sync() == 0 and fv is None and fn is out and fq.dtype == torch.float32
        assert np.array_equal(fn.cpu().numpy().view(np.uint32), net.astype(np.float32).view(np.uint32))
        assert np.array_equal(fq.cpu().numpy().view(np.uint32), q.astype(np.float32).view(np.uint32))
        nq, nv, nn, _ = n.run_sampled_impulses(30, 3, positions=False, velocities=False)
        assert nq is None and nv is None and _same(nn, net) and (net != 0).any()
        fh, fn_ = h.get_state(), n.get_state()
        assert _same(fh[0], fn_[0]) and _same(fh[1], fn_[1])
        on = torch.empty((10, 5, 4, 6), dtype=torch.float64, device="cuda")
        assert d.run_sampled_impulses_device(30, 3, positions=False, velocities=False, out_net=on) == (None, None, on)
        d.sync()


# ------------------------------------------------------------ 6. refusals
def test_refusals_step_nothing(rb, torch, monkeypatch):
    import ctypes as C
    with rb.BatchWorld.from_scenes(box_sweep()) as b:
        b.step(3)
        L, h = b._L, b._h
        E, M = b.n_envs, b.n_bodies
        sc = b.scene
        ok = (sc.dt, sc.restitution, sc.friction, sc.threshold)
        q, v, net = np.zeros((4, E, M, 7)), np.zeros((4, E, M, 6)), np.zeros((4, E, M, 6))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        dn = torch.zeros((4, E, M, 6), dtype=torch.float64, device="cuda")
        dp = C.c_void_p(dn.data_ptr())

        def unchanged():
            return np.array_equal(b.status()[1], np.full(E, 3)) and not net.any() and not q.any() and not bool(dn.any())
        host = lambda nsteps, every, pr, n: L.rb_batch_run_sampled_impulses(h, nsteps, every, *pr, p(q), p(v), n, None)
        dev = lambda nsteps, every, pr, n, io=0: L.rb_batch_run_sampled_impulses_dev(h, nsteps, every, *pr, None, None, n, io)
        assert host(12, 0, ok, p(net)) == EINVAL and dev(12, 0, ok, dp) == EINVAL          # every < 1
        assert host(-1, 3, ok, p(net)) == EINVAL and dev(-1, 3, ok, dp) == EINVAL          # nsteps < 0
        assert host(12, 3, ok, None) == EINVAL and b"net NULL" in L.rb_last_error()         # net NULL with S > 0
        assert dev(12, 3, ok, None) == EINVAL
        assert dev(12, 3, ok, p(net)) == EINVAL                                              # a host pointer
        assert dev(12, 3, ok, dp, 7) == EINVAL                                               # an unknown io_dtype
        for bad in ((float("nan"), 0.5, 0.5, 0.0), (0.0, 0.5, 0.5, 0.0), (-0.01, 0.5, 0.5, 0.0), (0.01, -1.0, 0.5, 0.0),
                    (0.01, 0.5, -0.5, 0.0), (0.01, 0.5, 0.5, -1.0), (0.01, float("nan"), 0.5, 0.0)):
            assert host(12, 3, bad, p(net)) == EINVAL and dev(12, 3, bad, dp) == EINVAL, bad
            nf = C.c_int64(-7)
            assert L.rb_batch_step(h, 1, *bad, C.byref(nf)) == EINVAL                        # as rb_batch_step refuses them
        assert unchanged()
        # nsteps < every: steps, and writes nothing
        assert host(2, 3, ok, None) == 0 and dev(2, 3, ok, None) == 0 and b.sync() == 0
        assert np.array_equal(b.status()[1], np.full(E, 7)) and not net.any() and not q.any()
    with rb.BatchWorld(__import__("rbhip").scenes.multi_sphere4(), 3) as b:
        b.set_contact_law("balls")
        with pytest.raises(rb.RbError) as ei:
            b.run_sampled_impulses(12, 3)
        assert ei.value.code == EUNSUPPORTED and not b.status()[1].any()
        with pytest.raises(rb.RbError) as ei:
            b.run_sampled_impulses_device(12, 3)
        assert ei.value.code == EUNSUPPORTED and not b.status()[1].any()
