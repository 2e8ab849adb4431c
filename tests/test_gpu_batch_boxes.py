"""Box stacks and mixed bodies in one environment of a batch
(rb_batch_create_mixed; batch_mixed_kernel, rb_batch_boxes.hip): every
environment steps bit-identically (uint64 words; no tolerance anywhere) to the
committed oracle run on that environment's own scene with max_partners 32, one
step at a time with its contact records read.  Every test asserts that the
oracle recorded the contact kinds it is about (17 sphere-box, 32..35 the
points of a clipped box-box face, 40 box-box edge-edge, 1..8 plane-box
corner, 16 sphere-sphere), so a run that merely falls through the air cannot
pass.  The bounds on record counts were checked on the CPU and are weaker than
what the oracle records."""
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EDOM = -33
EUNSUPPORTED = -95
BOX_KINDS = (17, 32, 33, 34, 35, 40)


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


def _same(a, b):
    """Bit identity as 64-bit words (the sign of zeros counts)."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _differing(q, v, rq, rv):
    return [k for k in range(q.shape[0]) if not (_same(q[k], rq[k]) and _same(v[k], rv[k]))]


def _frozen(d):
    for a in d.values():
        for x in (a if isinstance(a, tuple) else a.values() if isinstance(a, dict) else (a,)):
            for y in (x if isinstance(x, tuple) else (x,)):
                if isinstance(y, np.ndarray):
                    y.setflags(write=False)
    return d


def oracle_run(oracle, scs, q0, v0, steps, dtype="f64", xfrc=None, keep=(), every=False):
    """Environment k through the oracle on scs[k] (max_partners 32; xfrc[k] its
    applied forces), one step at a time.  Returns the final (E, M, 7) / (E, M,
    6) state, {t: (q, v)} for t in keep (every: for every step) and a Counter
    of the recorded contact kinds over all environments and steps."""
    q, v = np.array(q0, np.float64), np.array(v0, np.float64)
    keep = range(1, steps + 1) if every else keep
    kept = {t: (q.copy(), v.copy()) for t in keep}
    kinds = Counter()
    for k, sc in enumerate(scs):
        osc = oracle.OracleScene(sc, max_partners=32)
        xf = None if xfrc is None else xfrc[k]
        qq, vv = q[k], v[k]
        for t in range(1, steps + 1):
            qq, vv, (cnt, par, kin, dis) = oracle.step(osc, qq, vv, 1, dtype=dtype, xfrc=xf, record=True)
            assert cnt.max() <= 32
            kinds.update(kin.tolist())
            if t in kept:
                kept[t][0][k], kept[t][1][k] = qq, vv
        q[k], v[k] = qq, vv
    assert np.isfinite(q).all() and np.isfinite(v).all()
    return q, v, kept, kinds


def _plane_box(kinds):
    return sum(kinds[c] for c in range(1, 9))


def _assert_box_kinds(kinds, floor):
    """Every box-involved kind and a plane-box corner were recorded at least floor times."""
    low = {c: kinds[c] for c in BOX_KINDS if kinds[c] < floor}
    assert not low and _plane_box(kinds) >= floor, (low, _plane_box(kinds))


def _states(scs):
    return np.stack([sc.qpos0 for sc in scs]), np.stack([sc.qvel0 for sc in scs])


# ------------------------------------------------------------ the shapes
E_COL = 37           # M = 4, 16 environments per wave: two full waves and a part
E_RAG = 9            # M = 14, 4 environments per wave and 8 idle lanes: two full waves and one environment


def column_scenes(**kw):
    """box_pile(1, 1, 3, seed=s): three cubes and a sphere cap, with a
    restitution and a friction per environment."""
    from rbhip import scenes
    rng = np.random.default_rng(1133)
    e, mu = rng.uniform(0.0, 0.5, E_COL), rng.uniform(0.1, 0.9, E_COL)
    return [scenes.box_pile(1, 1, 3, seed=s).with_(restitution=float(e[s]), friction=float(mu[s]), **kw)
            for s in range(E_COL)]


def ragged_scenes():
    from rbhip import scenes
    return [scenes.box_pile(2, 2, 3, seed=s) for s in range(E_RAG)]


KEEP_COL = (7, 150, 263, 300)


@pytest.fixture(scope="module")
def column(oracle):
    """The column sweep and its oracle states after 7, 150, 263 and 300 steps
    (computed once, never modified)."""
    scs = column_scenes()
    assert scs[0].n == 4 and list(scs[0].kind) == [1, 1, 1, 0]
    q0, v0 = _states(scs)
    q, v, kept, kinds = oracle_run(oracle, scs, q0, v0, 300, keep=KEEP_COL)
    return _frozen(dict(scs=scs, q0=q0, v0=v0, ref=kept, kinds=kinds))


@pytest.fixture(scope="module")
def ragged(oracle):
    scs = ragged_scenes()
    assert scs[0].n == 14
    q0, v0 = _states(scs)
    q, v, kept, kinds = oracle_run(oracle, scs, q0, v0, 200, keep=(200,))
    return _frozen(dict(scs=scs, q0=q0, v0=v0, ref=kept, kinds=kinds))


# ------------------------------------------------------------ 1. the column sweep
def test_column_sweep_bit_exact(rb, oracle, column):
    """M = 4, E = 37 through from_scenes, 300 steps (two launches).  Seed 0
    with box_pile's own restitution and friction records 320 / 654 / 624 /
    514 / 302 / 284 contacts of kinds 17 / 32 / 33 / 34 / 35 / 40 and 893
    plane-box corners."""
    from rbhip import scenes
    sc0 = scenes.box_pile(1, 1, 3, seed=0)
    _, _, _, k0 = oracle_run(oracle, [sc0], sc0.qpos0[None], sc0.qvel0[None], 300)
    assert [k0[c] for c in BOX_KINDS] == [320, 654, 624, 514, 302, 284] and _plane_box(k0) == 893, k0
    _assert_box_kinds(column["kinds"], 1000)
    with rb.BatchWorld.from_scenes(column["scs"]) as b:
        assert b.n_envs == E_COL and b.n_bodies == 4
        assert b.step(300) == 0
        q, v = b.get_state()
        code, done = b.status()
    bad = _differing(q, v, *column["ref"][300])
    assert not bad, f"environments differing from the oracle: {bad}"
    assert not code.any() and (done == 300).all()


# ------------------------------------------------------------ 2. a ragged wave
def test_ragged_wave_bit_exact(rb, ragged):
    """M = 14, E = 9, 200 steps."""
    _assert_box_kinds(ragged["kinds"], 300)
    with rb.BatchWorld.from_scenes(ragged["scs"]) as b:
        assert b.step(200) == 0
        q, v = b.get_state()
    bad = _differing(q, v, *ragged["ref"][200])
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ 3. a full wave
def test_full_wave_bit_exact(rb, oracle):
    """M = 64 (16 columns of three cubes, each with a sphere cap): one
    environment per wave, E = 2 (the second with its own friction), 150 steps."""
    from rbhip import scenes
    sc = scenes.box_pile(4, 4, 3, seed=0, sphere_every=1)
    assert sc.n == 64
    scs = [sc, sc.with_(friction=0.3)]
    q0, v0 = _states(scs)
    rq, rv, _, kinds = oracle_run(oracle, scs, q0, v0, 150)
    _assert_box_kinds(kinds, 300)
    assert not _same(rq[0], rq[1])
    with rb.BatchWorld.from_scenes(scs) as b:
        assert b.step(150) == 0
        q, v = b.get_state()
    bad = _differing(q, v, rq, rv)
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ 4. a sphere pair inside a mixed environment
def _cube_and_two_spheres():
    """One cube of box_pile(1, 1, 1) and two spheres of r 0.1 that fall on it
    while they drift into each other."""
    from rbhip import scenes
    c = scenes.box_pile(1, 1, 1, sphere_every=0)
    assert c.n == 1
    kind = np.array([1, 0, 0], np.int32)
    mass = np.array([c.mass[0], scenes.M_SPHERE_R01, scenes.M_SPHERE_R01])
    inertia = np.array([c.inertia[0], [scenes.I_SPHERE_R01] * 3, [scenes.I_SPHERE_R01] * 3])
    size = np.array([c.size[0], [0.1, 0, 0], [0.1, 0, 0]])
    qpos = np.array([c.qpos0[0], [-0.098, 0.0, 1.0, 1, 0, 0, 0], [0.098, 0.01, 1.02, 1, 0, 0, 0]])
    qvel = np.array([c.qvel0[0], [0.05, 0, 0, 0, 0, 0], [-0.05, 0, 0, 0, 0, 0]])
    return c.with_(name="cube_two_spheres", kind=kind, mass=mass, inertia=inertia, size=size, qpos0=qpos, qvel0=qvel)


def test_sphere_pair_inside_a_mixed_environment(rb, oracle):
    """Kinds 16 (sphere-sphere) and 17 (sphere-box) in one environment, 300
    steps: 28 and 818 records in the oracle run of the scene; E = 5 replicas
    of it, each with its own friction."""
    sc = _cube_and_two_spheres()
    scs = [sc.with_(friction=0.2 + 0.1 * k) for k in range(5)]
    q0, v0 = _states(scs)
    _, _, _, k4 = oracle_run(oracle, [sc], q0[:1], v0[:1], 300)
    assert (k4[16], k4[17]) == (28, 818), k4
    rq, rv, _, kinds = oracle_run(oracle, scs, q0, v0, 300)
    assert kinds[16] >= 50 and kinds[17] >= 2000, kinds
    with rb.BatchWorld.from_scenes(scs) as b:
        assert b.step(300) == 0
        q, v = b.get_state()
    bad = _differing(q, v, rq, rv)
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ 5. a pair that enters range and touches in one step
def test_boxes_entering_range_every_step(rb, oracle):
    """The two approaching cubes of test_gpu_boxes.py as one environment (and
    a replica), every one of 150 steps compared: the cubes meet in the very
    step their bounding spheres first overlap, so a step-start orientation
    that is not refreshed every step shows."""
    from test_gpu_boxes import _approaching_boxes
    sc = _approaching_boxes()
    q0, v0 = _states([sc, sc])
    _, _, every, kinds = oracle_run(oracle, [sc, sc], q0, v0, 150, every=True)
    assert kinds[32] >= 2 and kinds[40] >= 2, kinds
    with rb.BatchWorld(sc, 2) as b:
        for t in range(1, 151):
            assert b.step(1) == 0
            q, v = b.get_state()
            assert _same(q, every[t][0]) and _same(v, every[t][1]), f"state differs at step {t}"


# ------------------------------------------------------------ 6. equal to a World
def test_one_environment_equals_a_world(rb, ragged):
    sc = ragged["scs"][3]
    with rb.World(sc, max_partners=32) as w:
        w.step(200)
        wq, wv = w.get_state()
    with rb.BatchWorld(sc, 1) as b:
        assert b.step(200) == 0
        q, v = b.get_state()
    assert _same(q[0], wq) and _same(v[0], wv)
    assert _same(wq, ragged["ref"][200][0][3])


# ------------------------------------------------------------ 7. fp32
@pytest.mark.parametrize("shape", ["column", "ragged"])
def test_f32_bit_exact(rb, oracle, shape):
    """Both shapes in fp32 against the fp32 oracle, 150 steps."""
    scs = column_scenes() if shape == "column" else ragged_scenes()
    q0, v0 = _states(scs)
    rq, rv, _, kinds = oracle_run(oracle, scs, q0, v0, 150, dtype="f32")
    _assert_box_kinds(kinds, 100)
    with rb.BatchWorld.from_scenes(scs, dtype="f32") as b:
        assert b.step(150) == 0
        q, v = b.get_state()
    bad = _differing(q, v, rq, rv)
    assert not bad, f"environments differing from the fp32 oracle: {bad}"


# ------------------------------------------------------------ 8. RAW normals
def test_raw_normals_bit_exact(rb, oracle, column):
    scs = column_scenes(normal_convention="raw")
    q0, v0 = _states(scs)
    rq, rv, _, kinds = oracle_run(oracle, scs, q0, v0, 300)
    _assert_box_kinds(kinds, 300)
    assert not _same(rq, column["ref"][300][0])              # the convention matters
    with rb.BatchWorld.from_scenes(scs) as b:
        assert b.step(300) == 0
        q, v = b.get_state()
    bad = _differing(q, v, rq, rv)
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ 9. the cut, and a reset of listed environments
def test_cut_independence_and_reset(rb, oracle, column):
    """step(300) == step(7) + step(256) + step(37) (the oracle's states at 7,
    263 and 300); set_state on environments {20, 3, 36} resets only those."""
    d, ref = column, column["ref"]
    with rb.BatchWorld.from_scenes(d["scs"]) as b:
        for n, t in ((7, 7), (256, 263), (37, 300)):
            assert b.step(n) == 0
            q, v = b.get_state()
            bad = _differing(q, v, *ref[t])
            assert not bad, f"after step {t}: environments differing from the oracle: {bad}"
        ids = [20, 3, 36]
        others = [k for k in range(E_COL) if k not in ids]
        b.set_state(d["q0"][ids], d["v0"][ids], envs=ids)
        code, done = b.status()
        assert not code.any() and (done[ids] == 0).all() and (done[others] == 300).all()
        gq, gv = b.get_state(envs=ids)
        assert _same(gq, d["q0"][ids]) and _same(gv, d["v0"][ids])
        assert b.step(7) == 0
        q, v = b.get_state()
        code, done = b.status()
        assert (done[ids] == 7).all() and (done[others] == 307).all()
    assert _same(q[ids], ref[7][0][ids]) and _same(v[ids], ref[7][1][ids])
    oq, ov, _, _ = oracle_run(oracle, [d["scs"][k] for k in others], ref[300][0][others], ref[300][1][others], 7)
    assert _same(q[others], oq) and _same(v[others], ov)


# ------------------------------------------------------------ 10. sampled runs
@pytest.mark.parametrize("velocities", [True, False])
def test_sampled_run(rb, column, velocities):
    """run_sampled(300, 7) (the REC instances; the second launch starts inside
    a sampling period) equals the step(7) + get_state() loop word for word and
    ends in the state of step(300)."""
    d = column
    S = 300 // 7
    with rb.BatchWorld.from_scenes(d["scs"]) as a:
        lq, lv = np.zeros((S, E_COL, 4, 7)), np.zeros((S, E_COL, 4, 6))
        for s in range(S):
            assert a.step(7) == 0
            lq[s], lv[s] = a.get_state()
    assert _same(lq[0], d["ref"][7][0]) and _same(lv[0], d["ref"][7][1])
    with rb.BatchWorld.from_scenes(d["scs"]) as b:
        sq, sv, nf = b.run_sampled(300, 7, velocities=velocities)
        fq, fv = b.get_state()
        code, done = b.status()
    assert nf == 0 and sq.shape == (S, E_COL, 4, 7)
    assert _same(sq, lq)
    assert _same(sv, lv) if velocities else sv is None
    assert _same(fq, d["ref"][300][0]) and _same(fv, d["ref"][300][1])
    assert not code.any() and (done == 300).all()


# ------------------------------------------------------------ 11. planes, gravity and forces per environment
def _env_knobs(E, M):
    """A ground tilted by up to 0.15 rad about a random horizontal axis,
    gravity (U(-0.5, 0.5), U(-0.5, 0.5), -9.8 U(0.7, 1.3)), forces ~ N(0, 5) N
    and torques ~ N(0, 0.5) N m on every body."""
    rng = np.random.default_rng(411)
    tilt, az = rng.uniform(0.0, 0.15, E), rng.uniform(0.0, 2 * np.pi, E)
    planes = np.zeros((E, 1, 6))
    planes[:, 0, 0], planes[:, 0, 1], planes[:, 0, 2] = np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)
    gravity = np.stack([rng.uniform(-0.5, 0.5, E), rng.uniform(-0.5, 0.5, E), -9.8 * rng.uniform(0.7, 1.3, E)], axis=1)
    xfrc = np.concatenate([rng.normal(0.0, 5.0, (E, M, 3)), rng.normal(0.0, 0.5, (E, M, 3))], axis=2)
    return planes, gravity, xfrc


def test_per_environment_planes_gravity_forces(rb, oracle, column):
    """The ENVS instances: the column sweep with a tilted ground, a gravity and
    applied forces and torques per environment (set_planes / set_gravity /
    set_xfrc), 300 steps against the oracle on each environment's scene."""
    planes, gravity, xfrc = _env_knobs(E_COL, 4)
    assert np.abs(xfrc[:, :, 0:3]).min() > 0 and np.abs(xfrc[:, :, 3:6]).min() > 0
    scs = [sc.with_(planes=planes[k], gravity=gravity[k]) for k, sc in enumerate(column["scs"])]
    rq, rv, _, kinds = oracle_run(oracle, scs, column["q0"], column["v0"], 300, xfrc=xfrc)
    _assert_box_kinds(kinds, 100)            # (the caps roll off the tilted stacks: 126 sphere-box records)
    assert not _same(rq, column["ref"][300][0])
    with rb.BatchWorld.from_scenes(column["scs"]) as b:
        b.set_planes(planes)
        b.set_gravity(gravity)
        b.set_xfrc(xfrc)
        assert b.step(300) == 0
        q, v = b.get_state()
    bad = _differing(q, v, rq, rv)
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ 12. sizes per environment
def test_per_environment_sizes(rb, oracle, column):
    """set_bodies gives the cubes of every environment their own non-cubic half
    extents (0.4 U(0.7, 1.0) per axis: they only shrink, so no stack starts
    overlapping) and the inertia of a cuboid of that shape; the oracle runs on
    the matching scenes."""
    rng = np.random.default_rng(1212)
    t = column["scs"][0]
    box = t.kind != 0
    size = np.broadcast_to(t.size, (E_COL, 4, 3)).copy()
    size[:, box] *= rng.uniform(0.7, 1.0, (E_COL, int(box.sum()), 3))
    mass = np.broadcast_to(t.mass, (E_COL, 4)).copy()
    inertia = np.broadcast_to(t.inertia, (E_COL, 4, 3)).copy()
    h2 = size[:, box] ** 2
    inertia[:, box] = mass[:, box, None] / 3.0 * np.stack([h2[..., 1] + h2[..., 2], h2[..., 0] + h2[..., 2],
                                                          h2[..., 0] + h2[..., 1]], axis=-1)
    scs = [sc.with_(size=size[k], inertia=inertia[k]) for k, sc in enumerate(column["scs"])]
    rq, rv, _, kinds = oracle_run(oracle, scs, column["q0"], column["v0"], 300)
    _assert_box_kinds(kinds, 300)
    assert not _same(rq, column["ref"][300][0])
    with rb.BatchWorld.from_scenes(column["scs"]) as b:
        b.set_bodies(mass=mass, inertia=inertia, size=size)
        b.set_state(column["q0"], column["v0"])
        assert b.step(300) == 0
        q, v = b.get_state()
    bad = _differing(q, v, rq, rv)
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ 13. failure stays per environment
def test_failure_stays_per_environment(rb, column):
    """Environment 17 gets a gravity that carries it out of the domain of the
    position check within 40 steps: it alone reports RB_EDOM with the steps it
    completed and is frozen inside the domain; every other environment, those
    of its wave (16..31) included, equals its oracle run.

    The check refuses |x| / cell >= 2^29 with cell = 4 rmax 1.001 and rmax =
    0.4 sqrt(3), a cube's bounding radius: L = 2^29 cell.  Along y nothing but
    friction acts against gravity, and N semi-implicit steps of dt carry a
    body G dt^2 N (N + 1) / 2 >= G T^2 / 2 (T = N dt): G = 4 L / T^2 leaves
    the domain with a factor 2 to spare."""
    d = column
    N, dt = 150, d["scs"][0].dt
    L = 2.0 ** 29 * 4 * (0.4 * np.sqrt(3.0)) * 1.001
    G = 4.0 * L / (N * dt) ** 2
    gravity = np.stack([sc.gravity for sc in d["scs"]])
    gravity[17] = [0.0, G, -9.8]
    others = [k for k in range(E_COL) if k != 17]
    with rb.BatchWorld.from_scenes(d["scs"]) as b:
        b.set_gravity(gravity)
        assert b.step(N) == 1
        code, done = b.status()
        q, v = b.get_state()
    assert code[17] == EDOM and 0 < done[17] < N
    assert not code[others].any() and (done[others] == N).all()
    assert np.isfinite(q[17]).all() and np.abs(q[17, :, 0:3]).max() < L
    rq, rv = d["ref"][150]
    assert _same(q[others], rq[others]) and _same(v[others], rv[others])


# ------------------------------------------------------------ 14. refusals
def test_two_ball_law_is_refused(rb, column):
    """The two-ball law takes spheres only: RB_EUNSUPPORTED at construction
    and from set_contact_law, after which the batch steps as before."""
    from rbhip import scenes
    with pytest.raises(rb.RbError) as ei:
        rb.BatchWorld(scenes.box_pile(1, 1, 3), 3, law="balls")
    assert ei.value.code == EUNSUPPORTED
    with rb.BatchWorld.from_scenes(column["scs"]) as b:
        with pytest.raises(rb.RbError, match="spheres only") as ei:
            b.set_contact_law("balls")
        assert ei.value.code == EUNSUPPORTED
        assert b.step(7) == 0
        q, v = b.get_state()
    assert not _differing(q, v, *column["ref"][7])
