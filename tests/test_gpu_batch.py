"""Batched worlds (rbhip.BatchWorld, rb_batch_*): every environment of a
batch steps bit-identically (uint64 words; no tolerance anywhere) to the
committed oracle run on that environment's own scene and parameters, or to a
committed golden of the reference."""
import numpy as np
import pytest

from conftest import golden_scene, load_golden

pytestmark = pytest.mark.gpu

EDOM = -33


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


def _same(a, b):
    """Bit identity as 64-bit words (the sign of zeros counts)."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _oracle_envs(oracle, scs, q, v, steps, dtype="f64", keep=(), max_partners=16):
    """Each environment k through the oracle on its own scene scs[k], one
    step at a time so every step's recorded contact list is seen.  Returns
    the final (E, M, 7) / (E, M, 6) state, the states after the step counts
    in `keep`, and the number of sphere-sphere records over all steps."""
    q, v = np.array(q, np.float64), np.array(v, np.float64)
    kept = {t: (q.copy(), v.copy()) for t in keep}
    ss = 0
    for k, sc in enumerate(scs):
        osc = oracle.OracleScene(sc, max_partners=max_partners)
        qq, vv = q[k], v[k]
        for t in range(1, steps + 1):
            qq, vv, (cnt, par, kin, dis) = oracle.step(osc, qq, vv, 1, dtype=dtype, record=True)
            ss += int((kin == 16).sum())
            if t in kept:
                kept[t][0][k], kept[t][1][k] = qq, vv
        q[k], v[k] = qq, vv
    return q, v, kept, ss


# ------------------------------------------------------------ the four-ball batch
E4 = 37          # 16 environments per wave: two full waves and a part


def _four_ball_inputs():
    """multi_sphere4 with the balls moved together so that they meet: x, y =
    +-0.095 plus jitter +-0.01, z = 0.5 + 0.3 u, v ~ N(0, 0.3), w ~ N(0, 1);
    restitution in [0.2, 1] and friction in [0, 0.8] per environment."""
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
    e = rng.uniform(0.2, 1.0, E4)
    mu = rng.uniform(0.0, 0.8, E4)
    return sc, q, v, e, mu


@pytest.fixture(scope="module")
def four(oracle):
    """The four-ball batch's inputs and its oracle states after 7, 20, 70 and
    300 steps (computed once, never modified)."""
    sc, q, v, e, mu = _four_ball_inputs()
    scs = [sc.with_(restitution=float(e[k]), friction=float(mu[k])) for k in range(E4)]
    q300, v300, kept, ss = _oracle_envs(oracle, scs, q, v, 300, keep=(7, 20, 70))
    assert np.isfinite(q300).all() and np.isfinite(v300).all()
    kept[300] = (q300, v300)
    for a, b in kept.values():
        a.setflags(write=False)
        b.setflags(write=False)
    return dict(sc=sc, scs=scs, q=q, v=v, e=e, mu=mu, ref=kept, ss=ss)


def _four_batch(rb, four, dtype="f64"):
    b = rb.BatchWorld(four["sc"], E4, dtype=dtype)
    b.set_params(restitution=four["e"], friction=four["mu"])
    b.set_state(four["q"], four["v"])
    return b


def test_four_balls_ragged_batch_bit_exact(rb, four):
    """37 environments of four balls, each with its own restitution, friction
    and state, 300 steps (two launches): every environment bit-identical to
    the oracle, and the oracle's recorded lists show the balls met."""
    assert four["ss"] >= 100, four["ss"]
    with _four_batch(rb, four) as b:
        assert b.step(300) == 0
        q, v = b.get_state()
        code, done = b.status()
    rq, rv = four["ref"][300]
    bad = [k for k in range(E4) if not (_same(q[k], rq[k]) and _same(v[k], rv[k]))]
    assert not bad, f"environments differing from the oracle: {bad}"
    assert not code.any() and (done == 300).all()


def test_four_balls_f32_bit_exact(rb, oracle, four):
    """The same batch in fp32 against the fp32 oracle, 150 steps."""
    rq, rv, _, ss = _oracle_envs(oracle, four["scs"], four["q"], four["v"], 150, dtype="f32")
    assert ss >= 100, ss
    with _four_batch(rb, four, dtype="f32") as b:
        assert b.step(150) == 0
        q, v = b.get_state()
    assert _same(q, rq) and _same(v, rv)


# ------------------------------------------------------------ goldens through the batch
@pytest.mark.parametrize("name", ["traj_single_sphere", "traj_single_cube"])
def test_single_body_goldens_in_a_batch(rb, name):
    """M = 1, E = 130 (two full waves and a part; the cube: box-plane corners
    on the incline).  Environments 0 and 129 carry the golden's own state and
    equal it at every 100-step checkpoint; the others carry other velocities."""
    g = load_golden(name)
    sc = golden_scene(g)
    E = 130
    rng = np.random.default_rng(5)
    q = np.broadcast_to(sc.qpos0, (E, 1, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (E, 1, 6)).copy()
    v[1:E - 1] += rng.normal(0.0, 0.5, (E - 2, 1, 6))
    with rb.BatchWorld(sc, E) as b:
        b.set_state(q, v)
        for t in range(100, 2001, 100):
            assert b.step(100) == 0
            gq, gv = b.get_state(envs=[0, E - 1])
            for k in range(2):
                assert _same(gq[k, 0], g["qpos"][t]) and _same(gv[k, 0], g["qvel"][t]), f"{name}: differs after step {t}"
        aq, av = b.get_state()
    assert not _same(aq[1], aq[0]) and np.isfinite(aq).all() and np.isfinite(av).all()


@pytest.mark.parametrize("name", ["traj_multi4", "traj_flat64", "traj_flat64_raw"])
def test_nbody_goldens_in_a_batch(rb, name):
    """M = 4, and M = 64 (a full wave per environment) in both normal
    conventions; E = 3, environment 1 carries the golden's state and equals
    its snapshots at every snap_step."""
    g = load_golden(name)
    sc = golden_scene(g)
    M = sc.n
    rng = np.random.default_rng(6)
    q = np.broadcast_to(sc.qpos0, (3, M, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (3, M, 6)).copy()
    v[0, :, 0:3] += rng.normal(0.0, 0.3, (M, 3))
    v[2, :, 0:3] += rng.normal(0.0, 0.3, (M, 3))
    snaps = list(g["snap_step"])
    with rb.BatchWorld(sc, 3) as b:
        b.set_state(q, v)
        for si in range(1, len(snaps)):
            assert b.step(int(snaps[si] - snaps[si - 1])) == 0
            gq, gv = b.get_state(envs=[1])
            assert _same(gq[0], g["qpos"][si]) and _same(gv[0], g["qvel"][si]), f"{name}: differs at step {snaps[si]}"


# ------------------------------------------------------------ awkward M
@pytest.mark.parametrize("nx,ny,min_ss", [(3, 1, 5), (11, 3, 50)])
def test_awkward_bodies_per_environment(rb, oracle, nx, ny, min_ss):
    """M = 3 (21 environments per wave, one idle lane) and M = 33 (one
    environment per wave, 31 idle lanes): 5 jittered environments of a packed
    grid (spacing 0.19 < 2 r), 200 steps, against the oracle."""
    from rbhip import scenes
    sc = scenes.flat_spheres(nx, ny, spacing=0.19)
    E, M = 5, sc.n
    rng = np.random.default_rng(11)
    q = np.broadcast_to(sc.qpos0, (E, M, 7)).copy()
    v = np.broadcast_to(sc.qvel0, (E, M, 6)).copy()
    q[:, :, 0:3] += rng.uniform(-0.02, 0.02, (E, M, 3))
    v[:, :, 0:3] += rng.normal(0.0, 0.3, (E, M, 3))
    rq, rv, _, ss = _oracle_envs(oracle, [sc] * E, q, v, 200)
    assert ss >= min_ss, ss
    with rb.BatchWorld(sc, E) as b:
        b.set_state(q, v)
        assert b.step(200) == 0
        gq, gv = b.get_state()
    assert _same(gq, rq) and _same(gv, rv)


# ------------------------------------------------------------ more partners than a World allows
def test_more_partners_than_a_world_allows(rb, oracle):
    """24 spheres of r 0.1 within +-0.03 of one point: 23 partners per body
    (the oracle needs max_partners = 32; a batch has no partner list).  E = 2,
    50 steps."""
    from rbhip import scenes
    sc = scenes.flat_spheres(6, 4)
    E, M = 2, sc.n
    rng = np.random.default_rng(12)
    q = np.zeros((E, M, 7))
    q[:, :, 0:3] = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.03, 0.03, (E, M, 3))
    q[:, :, 3] = 1.0
    v = np.broadcast_to(sc.qvel0, (E, M, 6)).copy()
    cnt = oracle.contacts(oracle.OracleScene(sc, max_partners=32), q[0])[0]
    assert (cnt == 23).all()
    with pytest.raises(RuntimeError, match="EOVERFLOW"):
        oracle.step(oracle.OracleScene(sc), q[0], v[0], 1)
    rq, rv, _, ss = _oracle_envs(oracle, [sc] * E, q, v, 50, max_partners=32)
    assert ss > 0
    with rb.BatchWorld(sc, E) as b:
        b.set_state(q, v)
        assert b.step(50) == 0
        gq, gv = b.get_state()
    assert _same(gq, rq) and _same(gv, rv)


# ------------------------------------------------------------ per-environment bodies
def test_per_environment_bodies(rb, oracle, four):
    """set_bodies: another radius, mass and inertia in every environment of
    the four-ball batch, against the oracle on each environment's scene."""
    sc = four["sc"]
    rng = np.random.default_rng(13)
    r = rng.uniform(0.08, 0.12, (E4, 4))
    mass = sc.mass[None, :] * rng.uniform(0.5, 2.0, (E4, 4))
    inertia = sc.inertia[None, :, :] * rng.uniform(0.5, 2.0, (E4, 4, 1)) * np.array([1.0, 1.1, 0.9])
    size = np.zeros((E4, 4, 3))
    size[:, :, 0] = r
    scs = [four["scs"][k].with_(mass=mass[k], inertia=inertia[k], size=size[k]) for k in range(E4)]
    rq, rv, _, ss = _oracle_envs(oracle, scs, four["q"], four["v"], 120)
    assert ss >= 50, ss
    assert not _same(rq, four["ref"][300][0])
    with _four_batch(rb, four) as b:
        b.set_bodies(mass=mass, inertia=inertia, size=size)
        assert b.step(120) == 0
        q, v = b.get_state()
    bad = [k for k in range(E4) if not (_same(q[k], rq[k]) and _same(v[k], rv[k]))]
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ cutting and reset
def test_cutting_and_reset(rb, oracle, four):
    """step(7) + step(13) == step(20) == the oracle's 300-step run at step
    20; a mid-run set_state of environments {20, 3} leaves every other
    environment's bits alone and restarts those two."""
    ref = four["ref"]
    with _four_batch(rb, four) as a, _four_batch(rb, four) as b:
        assert a.step(7) == 0
        q7, v7 = a.get_state()
        assert _same(q7, ref[7][0]) and _same(v7, ref[7][1])
        assert a.step(13) == 0 and b.step(20) == 0
        qa, va = a.get_state()
        qb, vb = b.get_state()
        assert _same(qa, qb) and _same(va, vb)
        assert _same(qa, ref[20][0]) and _same(va, ref[20][1])
        # a: on to step 300 in one call (the launches are cut elsewhere now)
        assert a.step(280) == 0
        qa, va = a.get_state()
        assert _same(qa, ref[300][0]) and _same(va, ref[300][1])
        # b: reset two environments at step 20
        ids = [20, 3]
        rng = np.random.default_rng(14)
        nq = four["q"][ids].copy()
        nv = four["v"][ids].copy()
        nq[:, :, 2] += 0.1
        nv[:, :, 0:3] += rng.normal(0.0, 0.2, (2, 4, 3))
        b.set_state(nq, nv, envs=ids)
        q1, v1 = b.get_state()
        others = [k for k in range(E4) if k not in ids]
        assert _same(q1[others], qb[others]) and _same(v1[others], vb[others])
        assert _same(q1[ids], nq) and _same(v1[ids], nv)
        code, done = b.status()
        assert not code.any() and (done[others] == 20).all() and (done[ids] == 0).all()
        assert b.step(50) == 0
        q2, v2 = b.get_state()
        code, done = b.status()
        assert (done[others] == 70).all() and (done[ids] == 50).all()
        assert _same(q2[others], ref[70][0][others]) and _same(v2[others], ref[70][1][others])
        rq, rv, _, _ = _oracle_envs(oracle, [four["scs"][k] for k in ids], nq, nv, 50)
        assert _same(q2[ids], rq) and _same(v2[ids], rv)
        # an environment id out of range is refused, and nothing changes
        for bad in ([E4], [-1], [0, E4 + 5]):
            with pytest.raises(rb.RbError, match="EINVAL"):
                b.set_state(nq[:len(bad)], nv[:len(bad)], envs=bad)
            with pytest.raises(rb.RbError, match="EINVAL"):
                b.get_state(envs=bad)
        q3, v3 = b.get_state()
        assert _same(q3, q2) and _same(v3, v2)


# ------------------------------------------------------------ failure isolation
def test_failure_is_per_environment(rb, four):
    """A NaN in one body of environment 5 fails that environment alone: it
    is not advanced, its status says RB_EDOM after 0 steps, the 36 others
    step exactly as without the fault; set_state with good data clears it."""
    ref = four["ref"]
    q = four["q"].copy()
    q[5, 2, 2] = np.nan
    others = [k for k in range(E4) if k != 5]
    with _four_batch(rb, four) as b:
        b.set_state(q, four["v"])
        assert b.step(20) == 1
        code, done = b.status()
        assert code[5] == EDOM and done[5] == 0
        assert not code[others].any() and (done[others] == 20).all()
        gq, gv = b.get_state()
        assert _same(gq[5], q[5]) and _same(gv[5], four["v"][5])          # unchanged, NaN and all
        assert _same(gq[others], ref[20][0][others]) and _same(gv[others], ref[20][1][others])
        # the C call with n_failed == NULL reports the failure (after stepping the rest)
        p = b._params(None, None, None, None)
        assert b._L.rb_batch_step(b._h, 1, *p, None) == EDOM
        code, done = b.status()
        assert done[5] == 0 and (done[others] == 21).all()
        # a World of environment 5's data fails the same way
        with rb.World(four["scs"][5].with_(qpos0=q[5], qvel0=four["v"][5])) as w:
            with pytest.raises(rb.RbError, match="EDOM"):
                w.step(1)
        # a reset with good data clears it
        b.set_state(four["q"][[5]], four["v"][[5]], envs=[5])
        code, done = b.status()
        assert not code.any() and done[5] == 0
        assert b.step(20) == 0
        gq, gv = b.get_state(envs=[5])
        assert _same(gq[0], ref[20][0][5]) and _same(gv[0], ref[20][1][5])
        code, done = b.status()
        assert not code.any() and done[5] == 20 and (done[others] == 41).all()
