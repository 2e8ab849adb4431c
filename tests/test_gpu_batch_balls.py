"""The two-ball law in a batch (BatchWorld(law="balls"),
rb_batch_set_contact_law) and sampled runs (BatchWorld.run_sampled,
rb_batch_run_sampled).  Every comparison is a bit comparison: uint64 words
against the committed oracle or against another batch, np.array_equal against
the goldens of the reference (whose signed zeros may differ)."""
import numpy as np
import pytest

from conftest import golden_scene, load_golden

pytestmark = pytest.mark.gpu

EDOM, EINVAL, EUNSUPPORTED = -33, -22, -95


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


def _same(a, b):
    """Bit identity as 64-bit words (the sign of zeros and NaNs count)."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _jitter(sc, E, seed):
    """E states of the scene: positions +-0.02, velocities + N(0, 0.3);
    restitution in [0.2, 1] and friction in [0, 0.8] per environment."""
    rng = np.random.default_rng(seed)
    q = np.broadcast_to(sc.qpos0, (E, sc.n, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (E, sc.n, 6)).copy()
    q[:, :, 0:3] += rng.uniform(-0.02, 0.02, (E, sc.n, 3))
    v[:, :, 0:3] += rng.normal(0.0, 0.3, (E, sc.n, 3))
    return q, v, rng.uniform(0.2, 1.0, E), rng.uniform(0.0, 0.8, E)


def _pair_envs(oracle, scs, q, v, steps, e, mu, dtype="f64", tol=0.01, count=False, **kw):
    """Each environment through oracle.pair_step on its own scene.  count:
    one step at a time, returning the pair records of all steps and the most
    partners any ball had."""
    q, v = np.array(q, np.float64), np.array(v, np.float64)
    records, most = 0, 0
    for k, sc in enumerate(scs):
        osc = oracle.OracleScene(sc)
        par = dict(restitution=float(e[k]), friction=float(mu[k]), tol=tol, dtype=dtype, **kw)
        if not count:
            q[k], v[k] = oracle.pair_step(osc, q[k], v[k], steps, **par)
            continue
        for _ in range(steps):
            q[k], v[k], (cnt, _p) = oracle.pair_step(osc, q[k], v[k], 1, record=True, **par)
            records += int(cnt.sum())
            most = max(most, int(cnt.max()))
    return (q, v, records, most) if count else (q, v)


def _ball_batch(rb, sc, q, v, e, mu, dtype="f64", law="balls"):
    b = rb.BatchWorld(sc, q.shape[0], dtype=dtype, law=law)
    b.set_params(restitution=e, friction=mu)
    b.set_state(q, v)
    return b


# ------------------------------------------------------------ 1. the reference's two-ball goldens
@pytest.mark.parametrize("name", ["traj_balls2", "traj_balls2_spin"])
def test_two_ball_goldens_in_a_batch(rb, name):
    """M = 2, E = 33 (a full wave of 32 environments and one more).
    Environments 0 and 32 carry the golden's state and equal it after every
    one of its 600 steps (one sampled run); the others carry other velocities."""
    g = load_golden(name)
    sc = golden_scene(g)
    E, T = 33, g["qpos"].shape[0]
    assert T == 600
    rng = np.random.default_rng(21)
    q = np.broadcast_to(sc.qpos0, (E, 2, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (E, 2, 6)).copy()
    v[1:E - 1, :, 0:3] += rng.normal(0.0, 0.3, (E - 2, 2, 3))
    with rb.BatchWorld(sc, E, law="balls", tol=float(g["tol"])) as b:
        b.set_state(q, v)
        sq, sv, nf = b.run_sampled(T, 1)
    assert nf == 0 and sq.shape == (T, E, 2, 7) and sv.shape == (T, E, 2, 6)
    for k in (0, E - 1):
        bad = [t for t in range(T) if not (np.array_equal(sq[t, k], g["qpos"][t]) and np.array_equal(sv[t, k], g["qvel"][t]))]
        assert not bad, f"{name}: environment {k} differs from the reference first after step {bad[0] + 1}"
    assert not _same(sq[-1, 1], sq[-1, 0]) and np.isfinite(sq).all() and np.isfinite(sv).all()
    # the same run cut into calls
    with rb.BatchWorld(sc, E, law="balls", tol=float(g["tol"])) as b:
        b.set_state(q, v)
        for k in (1, 99, 200, 300):
            assert b.step(k) == 0
        fq, fv = b.get_state()
    assert np.array_equal(fq[0], g["qpos"][-1]) and np.array_equal(fv[0], g["qvel"][-1])
    assert np.array_equal(fq[E - 1], g["qpos"][-1]) and np.array_equal(fv[E - 1], g["qvel"][-1])
    assert _same(fq, sq[-1]) and _same(fv, sv[-1])


# ------------------------------------------------------------ 2. N balls against the oracle
@pytest.fixture(scope="module")
def pile16(oracle):
    """balls_pile(4, 4): 5 jittered environments (four per wave: ragged), and
    the f64 oracle's 150-step run with its pair records."""
    from rbhip import scenes
    sc = scenes.balls_pile(4, 4, seed=2)
    q, v, e, mu = _jitter(sc, 5, 31)
    rq, rv, records, most = _pair_envs(oracle, [sc] * 5, q, v, 150, e, mu, count=True)
    for a in (q, v, e, mu, rq, rv):
        a.setflags(write=False)
    return dict(sc=sc, q=q, v=v, e=e, mu=mu, rq=rq, rv=rv, records=records, most=most)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ball_pile_batch_vs_oracle(rb, oracle, pile16, dtype):
    """M = 16, E = 5, own restitution / friction / state per environment, 150
    steps: every environment equals oracle.pair_step on its own scene."""
    p = pile16
    assert p["records"] >= 100 and p["most"] <= 16, (p["records"], p["most"])
    if dtype == "f64":
        rq, rv = p["rq"], p["rv"]
    else:
        rq, rv = _pair_envs(oracle, [p["sc"]] * 5, p["q"], p["v"], 150, p["e"], p["mu"], dtype="f32")
    with _ball_batch(rb, p["sc"], p["q"], p["v"], p["e"], p["mu"], dtype=dtype) as b:
        assert b.step(150) == 0
        q, v = b.get_state()
        code, done = b.status()
    bad = [k for k in range(5) if not (_same(q[k], rq[k]) and _same(v[k], rv[k]))]
    assert not bad, f"environments differing from the oracle: {bad}"
    assert not code.any() and (done == 150).all()


# ------------------------------------------------------------ 3. awkward M
@pytest.mark.parametrize("nx,ny,E,min_records", [(7, 9, 3, 100), (2, 2, 17, 1)])
def test_ball_law_awkward_bodies_per_environment(rb, oracle, nx, ny, E, min_records):
    """M = 63 (one environment per wave, one idle lane) and M = 4 with E = 17
    (16 environments per wave and one more), 120 steps, against the oracle."""
    from rbhip import scenes
    sc = scenes.balls_pile(nx, ny, seed=2)
    q, v, e, mu = _jitter(sc, E, 32)
    rq, rv, records, most = _pair_envs(oracle, [sc] * E, q, v, 120, e, mu, count=True)
    assert records >= min_records and most <= 16, (records, most)
    with _ball_batch(rb, sc, q, v, e, mu) as b:
        assert b.step(120) == 0
        gq, gv = b.get_state()
    bad = [k for k in range(E) if not (_same(gq[k], rq[k]) and _same(gv[k], rv[k]))]
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ 4. per-environment bodies
def test_ball_law_per_environment_bodies(rb, oracle, pile16):
    """set_bodies under the ball law: another radius and mass per environment,
    against pair_step on each environment's scene; the inertia rows are not
    read (the law derives I^-1 from m and r)."""
    p = pile16
    sc = p["sc"]
    rng = np.random.default_rng(33)
    r = rng.uniform(0.08, 0.12, (5, 16))
    mass = sc.mass[None, :] * rng.uniform(0.5, 2.0, (5, 16))
    size = np.zeros((5, 16, 3))
    size[:, :, 0] = r
    scs = [sc.with_(mass=mass[k], size=size[k]) for k in range(5)]
    rq, rv, records, most = _pair_envs(oracle, scs, p["q"], p["v"], 120, p["e"], p["mu"], count=True)
    assert records >= 50 and most <= 16, (records, most)
    assert not _same(rq, p["rq"])
    with _ball_batch(rb, sc, p["q"], p["v"], p["e"], p["mu"]) as b:
        b.set_bodies(mass=mass, size=size)
        assert b.step(120) == 0
        q, v = b.get_state()
    bad = [k for k in range(5) if not (_same(q[k], rq[k]) and _same(v[k], rv[k]))]
    assert not bad, f"environments differing from the oracle: {bad}"
    with _ball_batch(rb, sc, p["q"], p["v"], p["e"], p["mu"]) as b:
        b.set_bodies(mass=mass, size=size,
                     inertia=sc.inertia[None, :, :] * rng.uniform(0.5, 2.0, (5, 16, 1)) * np.array([1.0, 1.1, 0.9]))
        assert b.step(120) == 0
        q2, v2 = b.get_state()
    assert _same(q2, q) and _same(v2, v)


# ------------------------------------------------------------ 5. law switch, parameter change
def test_ball_law_switch_round_trip(rb, oracle, pile16):
    """mujoco -> balls -> mujoco on one batch, 20 steps each, continues each
    law's run (as test_gpu_balls.py::test_law_switch_round_trip for a world)."""
    p = pile16
    sc, E = p["sc"], 5
    q1, v1 = p["q"].copy(), p["v"].copy()
    scs = [sc.with_(restitution=float(p["e"][k]), friction=float(p["mu"][k])) for k in range(E)]
    for k in range(E):
        q1[k], v1[k] = oracle.step(oracle.OracleScene(scs[k]), q1[k], v1[k], 20)
    q2, v2 = _pair_envs(oracle, scs, q1, v1, 20, p["e"], p["mu"])
    q3, v3 = q2.copy(), v2.copy()
    for k in range(E):
        q3[k], v3[k] = oracle.step(oracle.OracleScene(scs[k]), q3[k], v3[k], 20)
    with _ball_batch(rb, sc, p["q"], p["v"], p["e"], p["mu"], law="mujoco") as b:
        assert b.step(20) == 0
        b.set_contact_law("balls", 0.01)
        assert b.step(20) == 0
        q, v = b.get_state()
        assert _same(q, q2) and _same(v, v2)
        b.set_contact_law("mujoco")
        assert b.step(20) == 0
        q, v = b.get_state()
    assert _same(q, q3) and _same(v, v3)


def test_ball_law_parameters_change_between_calls(rb, oracle, pile16):
    """30 steps, then 30 with dt = 0.005, e = 0.5, mu = 0.7: nothing of the
    ground phase is kept between calls."""
    p = pile16
    sc = p["sc"]
    q, v = np.array(p["q"]), np.array(p["v"])
    osc = oracle.OracleScene(sc)
    for k in range(5):
        q[k], v[k] = oracle.pair_step(osc, q[k], v[k], 30)
        q[k], v[k] = oracle.pair_step(osc, q[k], v[k], 30, dt=0.005, restitution=0.5, friction=0.7)
    with rb.BatchWorld(sc, 5, law="balls") as b:
        b.set_state(p["q"], p["v"])
        assert b.step(30) == 0
        assert b.step(30, dt=0.005, restitution=0.5, friction=0.7) == 0
        gq, gv = b.get_state()
    assert _same(gq, q) and _same(gv, v)


# ------------------------------------------------------------ 6. refusals
def test_ball_law_refusals(rb, pile16):
    from rbhip import scenes
    for sc in (scenes.single_cube(), scenes.incline_spheres(2, 2)):
        with pytest.raises(rb.RbError) as ei:
            rb.BatchWorld(sc, 3, law="balls")
        assert ei.value.code == EUNSUPPORTED
        with rb.BatchWorld(sc, 3) as b, rb.BatchWorld(sc, 3) as ref:
            with pytest.raises(rb.RbError) as ei:
                b.set_contact_law("balls")
            assert ei.value.code == EUNSUPPORTED
            assert b.step(10) == 0 and ref.step(10) == 0          # on in its previous law
            assert all(_same(x, y) for x, y in zip(b.get_state(), ref.get_state()))
    p = pile16
    for prev in ("mujoco", "balls"):
        with _ball_batch(rb, p["sc"], p["q"], p["v"], p["e"], p["mu"], law=prev) as b, \
                _ball_batch(rb, p["sc"], p["q"], p["v"], p["e"], p["mu"], law=prev) as ref:
            for law, tol in (("balls", -1.0), ("balls", float("nan")), ("mujoco", -1.0), (7, 0.01), (-1, 0.01)):
                with pytest.raises(rb.RbError) as ei:
                    b.set_contact_law(law, tol)
                assert ei.value.code == EINVAL, (law, tol)
            assert b.step(20) == 0 and ref.step(20) == 0
            assert all(_same(x, y) for x, y in zip(b.get_state(), ref.get_state()))


# ------------------------------------------------------------ the four-ball batch
E4 = 37          # 16 environments per wave: two full waves and a part


@pytest.fixture(scope="module")
def four():
    """multi_sphere4 with the balls moved together so that they meet (x, y =
    +-0.095 plus jitter, z = 0.5 + 0.3 u, v ~ N(0, 0.3), w ~ N(0, 1)), own
    restitution and friction per environment."""
    from rbhip import scenes
    sc = scenes.multi_sphere4()
    rng = np.random.default_rng(2024)
    q = np.zeros((E4, 4, 7))
    q[:, :, 0:2] = np.sign(sc.qpos0[:, 0:2]) * 0.095 + rng.uniform(-0.01, 0.01, (E4, 4, 2))
    q[:, :, 2] = 0.5 + 0.3 * rng.uniform(0.0, 1.0, (E4, 4))
    q[:, :, 3] = 1.0
    v = np.zeros((E4, 4, 6))
    v[:, :, 0:3] = rng.normal(0.0, 0.3, (E4, 4, 3))
    v[:, :, 3:6] = rng.normal(0.0, 1.0, (E4, 4, 3))
    e, mu = rng.uniform(0.2, 1.0, E4), rng.uniform(0.0, 0.8, E4)
    qn = q.copy()
    qn[5, 2, 2] = np.nan                 # the failing environment of tests 7 and 12
    for a in (q, v, e, mu, qn):
        a.setflags(write=False)
    return dict(sc=sc, q=q, v=v, e=e, mu=mu, q_nan=qn)


def _four_batch(rb, four, law="mujoco", q=None):
    return _ball_batch(rb, four["sc"], four["q"] if q is None else q, four["v"], four["e"], four["mu"], law=law)


@pytest.fixture(scope="module")
def four_loop(rb, four):
    """What sampled runs replace: step(7) + get_state(), 85 times, then on to
    step 600 (default law).  Computed once, never modified."""
    with _four_batch(rb, four) as b:
        qs, vs = [], []
        for _ in range(85):
            assert b.step(7) == 0
            q, v = b.get_state()
            qs.append(q)
            vs.append(v)
        assert b.step(5) == 0
        fq, fv = b.get_state()
        code, done = b.status()
    out = dict(q=np.stack(qs), v=np.stack(vs), fq=fq, fv=fv, code=code, done=done)
    for a in out.values():
        a.setflags(write=False)
    return out


# ------------------------------------------------------------ 7. failure isolation under the ball law
def test_ball_law_failure_is_per_environment(rb, four):
    others = [k for k in range(E4) if k != 5]
    with _four_batch(rb, four, law="balls") as clean, _four_batch(rb, four, law="balls", q=four["q_nan"]) as b:
        assert clean.step(20) == 0
        cq, cv = clean.get_state()
        assert b.step(20) == 1
        code, done = b.status()
        assert code[5] == EDOM and done[5] == 0
        assert not code[others].any() and (done[others] == 20).all()
        gq, gv = b.get_state()
        assert _same(gq[5], four["q_nan"][5]) and _same(gv[5], four["v"][5])     # unchanged, NaN and all
        assert _same(gq[others], cq[others]) and _same(gv[others], cv[others])
        assert not _same(cq, four["q"])
        b.set_state(four["q"][[5]], four["v"][[5]], envs=[5])
        code, done = b.status()
        assert not code.any() and done[5] == 0
        assert b.step(20) == 0
        gq, gv = b.get_state(envs=[5])
        assert _same(gq[0], cq[5]) and _same(gv[0], cv[5])
        code, done = b.status()
        assert not code.any() and done[5] == 20 and (done[others] == 40).all()


# ------------------------------------------------------------ 8. sampling equals the loop
@pytest.mark.parametrize("velocities", [True, False])
def test_sampled_run_equals_the_loop(rb, four, four_loop, velocities):
    """run_sampled(600, 7): three launches; step 259 is a sample inside the
    second.  All 85 samples, the final state, the status and steps_done equal
    the loop's."""
    with _four_batch(rb, four) as b:
        sq, sv, nf = b.run_sampled(600, 7, velocities=velocities)
        fq, fv = b.get_state()
        code, done = b.status()
    assert nf == 0 and sq.shape == (85, E4, 4, 7)
    bad = [s for s in range(85) if not _same(sq[s], four_loop["q"][s])]
    assert not bad, f"qpos samples differing from the loop: {bad}"
    if velocities:
        bad = [s for s in range(85) if not _same(sv[s], four_loop["v"][s])]
        assert not bad, f"qvel samples differing from the loop: {bad}"
    else:
        assert sv is None
    assert _same(fq, four_loop["fq"]) and _same(fv, four_loop["fv"])
    assert np.array_equal(code, four_loop["code"]) and np.array_equal(done, four_loop["done"]) and (done == 600).all()


# ------------------------------------------------------------ 9. goldens as curves
def test_multi4_golden_as_a_curve(rb):
    g = load_golden("traj_multi4")
    assert list(g["snap_step"]) == list(range(0, 401, 10))
    sc = golden_scene(g)
    rng = np.random.default_rng(6)
    q = np.broadcast_to(sc.qpos0, (3, 4, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (3, 4, 6)).copy()
    v[0, :, 0:3] += rng.normal(0.0, 0.3, (4, 3))
    v[2, :, 0:3] += rng.normal(0.0, 0.3, (4, 3))
    with rb.BatchWorld(sc, 3) as b:
        b.set_state(q, v)
        sq, sv, nf = b.run_sampled(400, 10)
    assert nf == 0 and sq.shape[0] == 40
    assert _same(sq[:, 1], g["qpos"][1:]) and _same(sv[:, 1], g["qvel"][1:])
    assert not _same(sq[:, 0], sq[:, 1])


@pytest.mark.parametrize("name", ["traj_single_sphere", "traj_single_cube"])
def test_single_body_goldens_as_curves(rb, name):
    """M = 1, E = 130 (the cube: the box-plane instance): environments 0 and
    129 against rows 100, 200, ..., 2000 of the golden."""
    g = load_golden(name)
    sc = golden_scene(g)
    E = 130
    rng = np.random.default_rng(5)
    q = np.broadcast_to(sc.qpos0, (E, 1, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (E, 1, 6)).copy()
    v[1:E - 1] += rng.normal(0.0, 0.5, (E - 2, 1, 6))
    with rb.BatchWorld(sc, E) as b:
        b.set_state(q, v)
        sq, sv, nf = b.run_sampled(2000, 100)
    assert nf == 0 and sq.shape == (20, E, 1, 7)
    rows = np.arange(100, 2001, 100)
    for k in (0, E - 1):
        assert _same(sq[:, k, 0], g["qpos"][rows]) and _same(sv[:, k, 0], g["qvel"][rows]), f"{name}: environment {k}"
    assert not _same(sq[:, 1], sq[:, 0]) and np.isfinite(sq).all() and np.isfinite(sv).all()


# ------------------------------------------------------------ 10. drains
def test_sampled_run_with_a_small_buffer(rb, four, four_loop, monkeypatch):
    """RBHIP_BATCH_SAMPLE_BYTES (read at creation) sized for exactly 3 samples
    of the four-ball batch: run_sampled(600, 7) drains 29 times and returns
    the same words.  With room for less than one sample: RB_EINVAL, and the
    state is unchanged."""
    per = E4 * 4 * 13 * (8 + 8)          # a sample with velocities, f64: its slot and its boundary rows
    monkeypatch.setenv("RBHIP_BATCH_SAMPLE_BYTES", str(3 * per))
    with _four_batch(rb, four) as b:
        sq, sv, nf = b.run_sampled(600, 7)
        fq, fv = b.get_state()
    assert nf == 0 and _same(sq, four_loop["q"]) and _same(sv, four_loop["v"])
    assert _same(fq, four_loop["fq"]) and _same(fv, four_loop["fv"])
    monkeypatch.setenv("RBHIP_BATCH_SAMPLE_BYTES", str(per - 1))
    with _four_batch(rb, four) as b:
        with pytest.raises(rb.RbError) as ei:
            b.run_sampled(600, 7)
        assert ei.value.code == EINVAL
        q, v = b.get_state()
        code, done = b.status()
        assert _same(q, four["q"]) and _same(v, four["v"]) and not code.any() and not done.any()
        # positions alone still fit
        sq, sv, nf = b.run_sampled(14, 7, velocities=False)
        assert nf == 0 and sv is None and _same(sq, four_loop["q"][:2])


# ------------------------------------------------------------ 11. edges
def test_sampled_run_edges(rb, four, four_loop):
    with _four_batch(rb, four) as b, _four_batch(rb, four) as ref:
        # every > nsteps: no sample, the state advanced by nsteps
        sq, sv, nf = b.run_sampled(5, 7)
        assert nf == 0 and sq.shape == (0, E4, 4, 7) and sv.shape == (0, E4, 4, 6)
        assert ref.step(5) == 0
        assert all(_same(x, y) for x, y in zip(b.get_state(), ref.get_state()))
        assert (b.status()[1] == 5).all()
        # nsteps = 0: a no-op
        sq, sv, nf = b.run_sampled(0, 1)
        assert nf == 0 and sq.shape[0] == 0
        assert all(_same(x, y) for x, y in zip(b.get_state(), ref.get_state()))
        assert (b.status()[1] == 5).all()
        # every = 0, nsteps < 0
        for nsteps, every in ((10, 0), (10, -3), (-1, 1)):
            with pytest.raises(rb.RbError) as ei:
                b.run_sampled(nsteps, every)
            assert ei.value.code == EINVAL
        assert b._L.rb_batch_run_sampled(b._h, 10, 5, *b._params(None, None, None, None), None, None, None) == EINVAL
        assert all(_same(x, y) for x, y in zip(b.get_state(), ref.get_state()))
    # samples exactly at the ends of launches
    with _four_batch(rb, four) as b, _four_batch(rb, four) as ref:
        sq, sv, nf = b.run_sampled(512, 256)
        assert nf == 0 and sq.shape[0] == 2
        for s in range(2):
            assert ref.step(256) == 0
            q, v = ref.get_state()
            assert _same(sq[s], q) and _same(sv[s], v)


# ------------------------------------------------------------ 12. a failing environment in a sampled run
def test_sampled_run_with_a_failing_environment(rb, four):
    others = [k for k in range(E4) if k != 5]
    with _four_batch(rb, four) as clean, _four_batch(rb, four, q=four["q_nan"]) as b:
        cq, cv, nf = clean.run_sampled(20, 5)
        assert nf == 0
        sq, sv, nf = b.run_sampled(20, 5)
        assert nf == 1 and sq.shape[0] == 4
        code, done = b.status()
        assert code[5] == EDOM and done[5] == 0 and (done[others] == 20).all()
    for s in range(4):
        assert _same(sq[s, 5], four["q_nan"][5]) and _same(sv[s, 5], four["v"][5]), f"sample {s}"
    assert _same(sq[:, others], cq[:, others]) and _same(sv[:, others], cv[:, others])
