"""Batches with a population (rb_batch_set_population; the kernels of
rb_batch_ragged.hip): per-environment body counts and kinds, the lanes of a
one-wave batch packed by body count.  Every environment steps bit-identically
(uint64 / uint32 words; no tolerance anywhere) to the committed oracle run on
that environment's own scene, the present bodies alone, with max_partners 32,
one step at a time with its contact records read.  Every test asserts that the
oracle recorded the contact kinds it is about (0 plane-sphere, 1..8 plane-box
corner, 16 sphere-sphere, 17 sphere-box, 32..35 the points of a clipped
box-box face, 40 box-box edge-edge), so a run that merely falls through the
air cannot pass.  The floors on record counts were checked on the CPU and are
far below what the oracle records."""
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EINVAL = -22
EDOM = -33
EUNSUPPORTED = -95
BOX_KINDS = (17, 32, 33, 34, 35, 40)
FIELDS = ("counts", "partner", "kind", "dist", "pos", "frame")
FLOAT_FIELDS = ("dist", "pos", "frame")


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


def _same(a, b):
    """Bit identity as 64-bit words (the sign of zeros and the payload of NaNs count)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def counts_of(scs):
    return np.array([sc.n for sc in scs], np.int32)


def padded_state(scs, M=None):
    """The scenes' initial states in the batch's (E, M, ...) layout, absent
    rows as from_ragged_scenes pads them."""
    M = max(sc.n for sc in scs) if M is None else M
    q, v = np.zeros((len(scs), M, 7)), np.zeros((len(scs), M, 6))
    q[:, :, 3] = 1.0
    for k, sc in enumerate(scs):
        q[k, :sc.n], v[k, :sc.n] = sc.qpos0, sc.qvel0
    return q, v


def oracle_run(oracle, scs, steps, dtype="f64", keep=(), start=None, xfrc=None):
    """Environment k through the oracle on scs[k] (max_partners 32) from its
    initial state (start: [(q, v)] per environment instead; xfrc[k]: applied
    forces of its bodies), one step at a time.  Returns {t: [(q, v) per
    environment]} for t in keep and steps, a Counter of the recorded contact
    kinds over all environments and steps, and the largest recorded count of
    one body in one step."""
    keep = sorted(set(keep) | {steps})
    kept = {t: [None] * len(scs) for t in keep}
    kinds, most = Counter(), 0
    for k, sc in enumerate(scs):
        osc = oracle.OracleScene(sc, max_partners=32)
        q, v = (sc.qpos0, sc.qvel0) if start is None else start[k]
        xf = None if xfrc is None else xfrc[k]
        for t in range(1, steps + 1):
            q, v, (cnt, par, kin, dis) = oracle.step(osc, q, v, 1, dtype=dtype, xfrc=xf, record=True)
            most = max(most, int(cnt.max()))
            kinds.update(kin.tolist())
            if t in kept:
                assert np.isfinite(q).all() and np.isfinite(v).all()
                q.setflags(write=False)
                v.setflags(write=False)
                kept[t][k] = (q, v)
    return kept, kinds, most


def differing(q, v, ref, scs, envs=None):
    """The environments whose present rows differ from the oracle's state ref
    ([(q, v)] per environment)."""
    return [k for k in (range(len(scs)) if envs is None else envs)
            if not (_same(q[k, :scs[k].n], ref[k][0]) and _same(v[k, :scs[k].n], ref[k][1]))]


def absent_mask(scs, M):
    return np.arange(M)[None, :] >= counts_of(scs)[:, None]


def plane_box(kinds):
    return sum(kinds[c] for c in range(1, 9))


def assert_box_kinds(kinds, floor):
    """Every box-involved kind and the plane-box corners were recorded at least floor times."""
    low = {c: kinds[c] for c in BOX_KINDS if kinds[c] < floor}
    assert not low and plane_box(kinds) >= floor, (low, plane_box(kinds))


# ------------------------------------------------------------ the ensembles
KEEP_1 = (7, 50, 100, 150, 263, 300)


def box_scenes():
    """Ensemble 1: body counts 1..8 over more than ten kind patterns, M = 8, 87 present
    bodies: two packed waves, environments 0..16 in 62 lanes, the rest in 25."""
    from rbhip import scenes
    return [scenes.box_pile(1 + (s // 3) % 2, 1, 1 + s % 3, seed=s, sphere_every=(0, 1, 3)[(s // 6) % 3])
            for s in range(24)]


def sphere_scenes():
    """Ensemble 2: spheres only, counts 1..12."""
    from rbhip import scenes
    return [scenes.flat_spheres(1 + s % 4, 1 + (s // 4) % 3, seed=s, spacing=0.19) for s in range(12)]


def wide_scenes(which):
    from rbhip import scenes
    p = scenes.box_pile
    if which == 0:      # counts 70, 30, 75, 14, 64, 65, 2: block 128, a whole idle wave in four of them
        return [p(4, 4, 4, seed=0), p(3, 3, 3, seed=1), p(5, 5, 3, seed=2, sphere_every=0), p(2, 2, 3, seed=3),
                p(4, 4, 4, seed=4, sphere_every=0), p(4, 4, 4, seed=5, sphere_every=16), p(1, 1, 1, seed=6)]
    # counts 147, 14, 70, 172: block 192
    return [p(7, 7, 3, seed=0, sphere_every=0), p(2, 2, 3, seed=1), p(4, 4, 4, seed=2), p(7, 7, 3, seed=3, sphere_every=2)]


@pytest.fixture(scope="module")
def boxes(oracle):
    """Ensemble 1 and its oracle states (computed once, never modified)."""
    scs = box_scenes()
    assert sorted(set(counts_of(scs))) == list(range(1, 9)) and counts_of(scs).sum() == 87
    assert len({tuple(sc.kind) for sc in scs}) >= 10           # (kind patterns)
    kept, kinds, most = oracle_run(oracle, scs, 300, keep=KEEP_1)
    assert most <= 32
    return dict(scs=scs, ref=kept, kinds=kinds)


@pytest.fixture(scope="module")
def spheres(oracle):
    scs = sphere_scenes()
    assert min(counts_of(scs)) == 1 and max(counts_of(scs)) == 12
    kept, kinds, most = oracle_run(oracle, scs, 200, keep=(60,))
    return dict(scs=scs, ref=kept, kinds=kinds)


@pytest.fixture(scope="module")
def wide0(oracle):
    scs = wide_scenes(0)
    assert counts_of(scs).tolist() == [70, 30, 75, 14, 64, 65, 2]
    kept, kinds, most = oracle_run(oracle, scs, 200, keep=(60,))
    return dict(scs=scs, ref=kept, kinds=kinds, most=most)


# ------------------------------------------------------------ 1. the box ensemble, packed
def test_box_ensemble_bit_exact(rb, boxes):
    """M = 8, E = 24, 300 steps compared after 7, 150, 263 and 300.  The
    oracle records each of kinds 17, 32, 33, 34, 35, 40 and the plane-box
    corners at least 2,700 times."""
    scs, ref = boxes["scs"], boxes["ref"]
    assert_box_kinds(boxes["kinds"], 500)
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        assert b.n_envs == 24 and b.n_bodies == 8
        n, kinds = b.population
        assert np.array_equal(n, counts_of(scs))
        done = 0
        for t in (7, 150, 263, 300):
            assert b.step(t - done) == 0
            done = t
            q, v = b.get_state()
            bad = differing(q, v, ref[t], scs)
            assert not bad, f"after step {t}: environments differing from the oracle: {bad}"
        code, steps = b.status()
    assert not code.any() and (steps == 300).all()


def test_box_ensemble_three_times_over(rb, boxes):
    """E = 72, five waves, one call of 300 steps (two launches): every copy equals the oracle."""
    scs = boxes["scs"] * 3
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        assert b.step(300) == 0
        q, v = b.get_state()
    bad = differing(q, v, boxes["ref"][300] * 3, scs)
    assert not bad, f"environments differing from the oracle: {bad}"
    assert _same(q[24:48], q[:24]) and _same(q[48:], q[:24]) and _same(v[24:48], v[:24]) and _same(v[48:], v[:24])


def test_box_ensemble_f32(rb, oracle):
    scs = box_scenes()
    kept, kinds, _ = oracle_run(oracle, scs, 200, dtype="f32")
    assert_box_kinds(kinds, 500)
    with rb.BatchWorld.from_ragged_scenes(scs, dtype="f32") as b:
        assert b.step(200) == 0
        q, v = b.get_state()
    bad = differing(q, v, kept[200], scs)
    assert not bad, f"environments differing from the fp32 oracle: {bad}"


# ------------------------------------------------------------ 2. the sphere ensemble (BOXES = false)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sphere_ensemble_bit_exact(rb, oracle, spheres, dtype):
    """Counts 1..12, 200 steps.  The oracle records kind 0 365 times and kind 16 118 times."""
    scs = spheres["scs"]
    kept, kinds = (spheres["ref"], spheres["kinds"]) if dtype == "f64" else oracle_run(oracle, scs, 200, dtype=dtype)[:2]
    assert kinds[0] >= 100 and kinds[16] >= 50, kinds
    with rb.BatchWorld.from_ragged_scenes(scs, dtype=dtype) as b:
        assert b.n_bodies == 12
        assert b.step(200) == 0
        q, v = b.get_state()
    bad = differing(q, v, kept[200], scs)
    assert not bad, f"environments differing from the oracle: {bad}"


def test_sphere_ensemble_with_a_full_wave(rb, oracle, spheres):
    """The same with one 64-sphere environment: M = 64, one environment fills a wave."""
    from rbhip import scenes
    big = scenes.flat_spheres(8, 8, spacing=0.19)
    scs = spheres["scs"][:5] + [big] + spheres["scs"][5:]
    kbig, kinds, _ = oracle_run(oracle, [big], 200)
    assert kinds[0] >= 100 and kinds[16] >= 50, kinds
    ref = spheres["ref"][200][:5] + kbig[200] + spheres["ref"][200][5:]
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        assert b.n_bodies == 64 and b.scene is big
        assert b.step(200) == 0
        q, v = b.get_state()
    bad = differing(q, v, ref, scs)
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ 3. the reference's default-law scenes side by side
def test_reference_scenes_in_one_batch(rb, oracle):
    """single_sphere, single_cube and multi_sphere4 (dt 0.009, threshold 1e-4)
    with their own planes, gravity, restitution and friction, 300 steps."""
    from rbhip import scenes
    scs = [sc.with_(dt=0.009, threshold=1e-4) for sc in (scenes.single_sphere(), scenes.single_cube(), scenes.multi_sphere4())]
    kept, kinds, _ = oracle_run(oracle, scs, 300)
    assert kinds[0] >= 10 and plane_box(kinds) >= 100, kinds
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        assert b.n_bodies == 4 and b.population[1][:, 0].tolist() == [0, 1, 0]
        assert b.step(300) == 0
        q, v = b.get_state()
    bad = differing(q, v, kept[300], scs)
    assert not bad, f"environments differing from the oracle: {bad}"


def test_kinds_per_environment_at_one_body(rb, oracle):
    """M = 1: cube_incline(a) and sphere_incline(a) alternating over 70
    angles, 64 environments per wave, two waves, 300 steps."""
    from rbhip import scenes
    angles = np.linspace(0.0, 0.7, 70)
    scs = [scenes.cube_incline(float(a)) if k % 2 == 0 else
           scenes.sphere_incline(float(a)).with_(threshold=1e-4, dt=scenes.cube_incline(0.0).dt) for k, a in enumerate(angles)]
    kept, kinds, _ = oracle_run(oracle, scs, 300)
    assert kinds[0] >= 100 and plane_box(kinds) >= 1000, kinds
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        assert b.n_bodies == 1 and b.population[1][:, 0].tolist() == [1, 0] * 35
        assert b.step(300) == 0
        q, v = b.get_state()
    bad = differing(q, v, kept[300], scs)
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ 4. wide
def test_wide_block_128(rb, wide0):
    """Counts 70, 30, 75, 14, 64, 65, 2: block 128, 200 steps.  The oracle's
    largest partner count is 10; kind 17 is recorded 1,420 times, every other
    box kind and the plane corners at least 2,600 times."""
    scs = wide0["scs"]
    assert wide0["most"] <= 32
    assert_box_kinds(wide0["kinds"], 200)
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        assert b.n_bodies == 75
        assert b.step(200) == 0
        q, v = b.get_state()
    bad = differing(q, v, wide0["ref"][200], scs)
    assert not bad, f"environments differing from the oracle: {bad}"


def test_wide_block_192(rb, oracle):
    """Counts 147, 14, 70, 172: block 192, 120 steps."""
    scs = wide_scenes(1)
    assert counts_of(scs).tolist() == [147, 14, 70, 172]
    kept, kinds, most = oracle_run(oracle, scs, 120)
    assert most <= 32
    assert_box_kinds(kinds, 200)
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        assert b.step(120) == 0
        q, v = b.get_state()
    bad = differing(q, v, kept[120], scs)
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ 5. a uniform population equals no population
@pytest.mark.parametrize("shape", ["one wave", "wide"])
def test_uniform_population_equals_none(rb, shape):
    """All counts M and the template's kinds: the same words after 200 steps
    as the batch without a population; clearing the population mid-run and
    setting it again changes nothing."""
    from rbhip import scenes
    scs = [scenes.box_pile(2, 2, 3, seed=s) for s in range(9)] if shape == "one wave" else \
          [scenes.box_pile(4, 4, 4, seed=s) for s in range(2)]
    E, M = len(scs), scs[0].n
    assert M == (14 if shape == "one wave" else 70)
    with rb.BatchWorld.from_scenes(scs) as a:
        assert a.population is None
        assert a.step(200) == 0
        aq, av = a.get_state()
    kinds = np.tile(scs[0].kind, (E, 1))
    with rb.BatchWorld.from_scenes(scs) as b:
        b.set_population(np.full(E, M), kinds)
        assert b.step(200) == 0
        bq, bv = b.get_state()
    assert _same(aq, bq) and _same(av, bv)
    with rb.BatchWorld.from_scenes(scs) as c:
        c.set_population(None, kinds)            # (counts default to M)
        assert c.step(70) == 0
        c.set_population(None, None)
        assert c.population is None
        assert c.step(60) == 0
        c.set_population(np.full(E, M), None)    # (kinds default to the template's)
        assert c.step(70) == 0
        cq, cv = c.get_state()
    assert _same(aq, cq) and _same(av, cv)


# ------------------------------------------------------------ 6. absent rows
def _garbage(scs, M):
    """The padded initial state with NaN positions (with a payload) and
    garbage velocities in the absent rows."""
    q, v = padded_state(scs, M)
    ab = absent_mask(scs, M)
    rng = np.random.default_rng(66)
    q[ab] = rng.normal(0.0, 1e3, (int(ab.sum()), 7))
    nan = np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0]
    q[ab, 0:3] = nan
    v[ab] = rng.normal(0.0, 1e6, (int(ab.sum()), 6))
    v[ab, 1] = np.inf
    return q, v, ab


def test_absent_rows_are_storage(rb, boxes):
    """NaN positions and garbage velocities in absent rows fail nothing, come
    back from get_state / get_state_device bit for bit and change no present word."""
    scs, ref = boxes["scs"], boxes["ref"]
    q0, v0, ab = _garbage(scs, 8)
    assert ab.sum() == 24 * 8 - 87
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        b.set_state(q0, v0)
        assert b.step(150) == 0
        q, v = b.get_state()
        dq, dv = b.get_state_device()
        assert b.sync() == 0
        dq, dv = dq.cpu().numpy(), dv.cpu().numpy()
        code, steps = b.status()
    assert not code.any() and (steps == 150).all()
    assert _same(q[ab], q0[ab]) and _same(v[ab], v0[ab])
    assert _same(dq, q) and _same(dv, v)
    bad = differing(q, v, ref[150], scs)
    assert not bad, f"environments differing from the oracle: {bad}"


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_sampled_runs_hold_zeros_in_absent_rows(rb, boxes, device):
    """run_sampled / run_sampled_device with every 7 over 50 steps equal the
    step(7) + get_state loop on present rows and hold zeros on absent rows
    (whose state rows hold NaNs and garbage)."""
    scs = boxes["scs"]
    q0, v0, ab = _garbage(scs, 8)
    S = 50 // 7
    with rb.BatchWorld.from_ragged_scenes(scs) as a:
        a.set_state(q0, v0)
        lq, lv = np.zeros((S, 24, 8, 7)), np.zeros((S, 24, 8, 6))
        for s in range(S):
            assert a.step(7) == 0
            lq[s], lv[s] = a.get_state()
        assert a.step(50 - 7 * S) == 0
        fq, fv = a.get_state()
    assert not differing(lq[0], lv[0], boxes["ref"][7], scs) and not differing(fq, fv, boxes["ref"][50], scs)
    lq[:, ab], lv[:, ab] = 0.0, 0.0
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        b.set_state(q0, v0)
        if device:
            sq, sv = b.run_sampled_device(50, 7)
            assert b.sync() == 0
            sq, sv = sq.cpu().numpy(), sv.cpu().numpy()
        else:
            sq, sv, nf = b.run_sampled(50, 7)
            assert nf == 0
        q, v = b.get_state()
    assert sq.shape == (S, 24, 8, 7) and _same(sq, lq) and _same(sv, lv)
    assert not np.ascontiguousarray(sq[:, ab]).view(np.uint64).any() and not np.ascontiguousarray(sv[:, ab]).view(np.uint64).any()
    assert _same(q, fq) and _same(v, fv)


# ------------------------------------------------------------ 7. failure isolation under packing
def test_failure_stays_per_environment_under_packing(rb, boxes):
    """A present body out of range in environment 5 (lanes 12..17 of the first
    packed wave) freezes environment 5 at its start state and no other
    environment, those of its wave included."""
    scs, ref = boxes["scs"], boxes["ref"]
    assert scs[5].n == 6
    q0, v0 = padded_state(scs, 8)
    q0[5, 3, 0] = 1e30
    others = [k for k in range(24) if k != 5]
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        b.set_state(q0, v0)
        assert b.step(7) == 1
        code, steps = b.status()
        q, v = b.get_state()
    assert code[5] == EDOM and steps[5] == 0
    assert not code[others].any() and (steps[others] == 7).all()
    assert _same(q[5], q0[5]) and _same(v[5], v0[5])
    bad = differing(q, v, ref[7], scs, envs=others)
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ 8. the population changes mid-run
def test_population_changes_mid_run(rb, oracle, boxes):
    """After 50 steps environment 14 (three cubes and a sphere cap) shrinks to two bodies and the top
    box of environment 2 (a column of three) becomes a sphere of radius 0.3
    (set_bodies gives its size row): 50 more steps equal the oracle continued
    on the changed scenes from the same state."""
    scs, ref = list(boxes["scs"]), boxes["ref"]
    assert scs[14].n == 4 and list(scs[14].kind) == [1, 1, 1, 0] and list(scs[2].kind) == [1, 1, 1]
    s4, s2 = scs[14], scs[2]
    scs[14] = s4.with_(kind=s4.kind[:2], mass=s4.mass[:2], inertia=s4.inertia[:2], size=s4.size[:2], qpos0=s4.qpos0[:2],
                      qvel0=s4.qvel0[:2])
    size2 = s2.size.copy()
    size2[2] = [0.3, 0.0, 0.0]
    scs[2] = s2.with_(kind=np.array([1, 1, 0], np.int32), size=size2)
    start = [(qv[0][:sc.n], qv[1][:sc.n]) for qv, sc in zip(ref[50], scs)]
    kept, kinds, _ = oracle_run(oracle, scs, 50, start=start)
    assert kinds[17] >= 10, kinds
    assert not _same(kept[50][2][0], ref[100][2][0]) and not _same(kept[50][14][0], ref[100][14][0][:2])    # the changes matter
    with rb.BatchWorld.from_ragged_scenes(boxes["scs"]) as b:
        assert b.step(50) == 0
        n, kinds_now = b.population
        size = np.tile(b.scene.size, (24, 1, 1))             # (absent rows: the template's, as from_ragged_scenes pads)
        for k, sc in enumerate(boxes["scs"]):
            size[k, :sc.n] = sc.size
        n[14] = 2
        kinds_now[2, 2] = 0
        size[2, 2] = [0.3, 0.0, 0.0]
        b.set_population(n, kinds_now)
        b.set_bodies(size=size)
        q50, v50 = b.get_state()
        assert not differing(q50, v50, ref[50], boxes["scs"])          # no state was converted
        assert b.step(50) == 0
        q, v = b.get_state()
        code, steps = b.status()
    assert not code.any() and (steps == 100).all()
    bad = differing(q, v, kept[50], scs)
    assert not bad, f"environments differing from the oracle: {bad}"
    assert _same(q[14, 2:], q50[14, 2:]) and _same(v[14, 2:], v50[14, 2:])     # the rows that became absent are never stored


# ------------------------------------------------------------ 9. planes, gravity and forces per environment
def test_per_environment_planes_gravity_forces(rb, oracle, boxes):
    """Ensemble 1 with a tilted ground, a gravity and applied forces and
    torques per environment (zeros in absent rows), 200 steps."""
    scs = boxes["scs"]
    E, M = 24, 8
    rng = np.random.default_rng(411)
    tilt, az = rng.uniform(0.0, 0.15, E), rng.uniform(0.0, 2 * np.pi, E)
    planes = np.zeros((E, 1, 6))
    planes[:, 0, 0], planes[:, 0, 1], planes[:, 0, 2] = np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)
    gravity = np.stack([rng.uniform(-0.5, 0.5, E), rng.uniform(-0.5, 0.5, E), -9.8 * rng.uniform(0.7, 1.3, E)], axis=1)
    xfrc = np.concatenate([rng.normal(0.0, 5.0, (E, M, 3)), rng.normal(0.0, 0.5, (E, M, 3))], axis=2)
    xfrc[absent_mask(scs, M)] = 0.0
    tilted = [sc.with_(planes=planes[k], gravity=gravity[k]) for k, sc in enumerate(scs)]
    kept, kinds, _ = oracle_run(oracle, tilted, 200, xfrc=[xfrc[k, :sc.n] for k, sc in enumerate(scs)])
    # (the caps roll off the tilted stacks: 32 sphere-box records)
    assert all(kinds[c] >= 500 for c in (32, 33, 34, 35, 40)) and kinds[17] >= 20 and plane_box(kinds) >= 500, kinds
    assert not _same(kept[200][11][0], boxes["ref"][150][11][0])
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        b.set_planes(planes)
        b.set_gravity(gravity)
        b.set_xfrc(xfrc)
        assert b.step(200) == 0
        q, v = b.get_state()
    bad = differing(q, v, kept[200], scs)
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ 10. the contact query
def _dense(lists, n, M, R):
    """oracle.contacts()' CSR lists of the n present bodies in the query's
    dense layout over M slots: absent bodies count 0, unused slots kind -1 and zeros."""
    cnt, par, kin, dis, pos, frm = lists
    out = dict(counts=np.zeros(M, np.int32), partner=np.zeros((M, R), np.int32), kind=np.full((M, R), -1, np.int32),
               dist=np.zeros((M, R)), pos=np.zeros((M, R, 3)), frame=np.zeros((M, R, 3)))
    out["counts"][:n] = cnt
    at = 0
    for b in range(n):
        k = min(int(cnt[b]), R)
        for name, src in (("partner", par), ("kind", kin), ("dist", dis), ("pos", pos), ("frame", frm)):
            out[name][b, :k] = src[at:at + k]
        at += int(cnt[b])
    return out


def _query_differs(con, ref):
    bad = []
    for name in FIELDS:
        got, want = getattr(con, name), ref[name]
        got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
        if name in FLOAT_FIELDS:
            same = _same(got, want)
        else:
            same = got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
        if not same:
            bad.append(name)
    return bad


@pytest.mark.parametrize("which", ["boxes", "spheres", "wide"])
def test_contact_query(rb, oracle, request, which):
    """contacts() and contacts_device() after 0 and 60 steps equal
    oracle.contacts of each environment's scene on present bodies, records and
    geometry; absent bodies have count 0 and unused slots only; a counts-only
    query agrees."""
    scs = request.getfixturevalue({"boxes": "boxes", "spheres": "spheres", "wide": "wide0"}[which])["scs"]
    E, M, R = len(scs), max(sc.n for sc in scs), 16
    ab = absent_mask(scs, M)
    listed = Counter()
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        for t in (0, 60):
            if t:
                assert b.step(60) == 0
            q, _ = b.get_state()
            per = []
            for k, sc in enumerate(scs):
                lists = oracle.contacts(oracle.OracleScene(sc, max_partners=32), q[k, :sc.n])
                listed.update(lists[2].tolist())
                per.append(_dense(lists, sc.n, M, R))
            ref = {name: np.stack([p[name] for p in per]) for name in FIELDS}
            con = b.contacts(max_records=R)
            assert not _query_differs(con, ref), (which, t)
            assert con.truncated == int((ref["counts"] > R).sum())
            assert not con.counts[ab].any() and (con.kind[ab] == -1).all() and not con.partner[ab].any()
            assert not np.ascontiguousarray(con.pos[ab]).view(np.uint64).any()
            dev = b.contacts_device(max_records=R)
            only = b.contacts_device(max_records=0)
            assert b.sync() == 0
            assert not _query_differs(dev, ref), (which, t)
            assert np.array_equal(only.counts.cpu().numpy(), ref["counts"]) and only.partner is None
            assert np.array_equal(b.contacts(max_records=0).counts, ref["counts"])
            # a list of environments, out of order
            ids = [E - 1, 0, E // 2]
            some = b.contacts(envs=ids, max_records=R)
            assert not _query_differs(some, {name: ref[name][ids] for name in FIELDS})
    if which == "spheres":
        assert listed[0] >= 1 and listed[16] >= 5, listed
    else:
        assert all(listed[c] >= 1 for c in (17, 32, 33)) and plane_box(listed) >= 20, listed


def test_contact_query_of_a_failed_environment(rb, boxes):
    """A failed environment reports -1 for all M slots, absent ones included."""
    scs = boxes["scs"]
    q0, v0 = padded_state(scs, 8)
    q0[5, 3, 0] = 1e30
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        b.set_state(q0, v0)
        assert b.step(1) == 1
        con = b.contacts(max_records=4)
    assert (con.counts[5] == -1).all() and (con.kind[5] == -1).all()
    assert (con.counts[[4, 6]] >= 0).all() and not con.counts[absent_mask(scs, 8) & (np.arange(24) != 5)[:, None]].any()


# ------------------------------------------------------------ 11. refusals
def test_refusals_change_nothing(rb, boxes):
    """RB_EINVAL: a count of 0 or M + 1, a bad kind in an absent slot.
    RB_EUNSUPPORTED: set_contact_law("balls") with a population set.  Each
    leaves the next 20 steps identical to a batch that never saw the call."""
    scs = boxes["scs"]
    with rb.BatchWorld.from_ragged_scenes(scs) as a:
        assert a.step(27) == 0
        want = a.get_state()
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        assert b.step(7) == 0
        n, kinds = b.population
        for bad_n, bad_k, what in ((np.where(np.arange(24) == 3, 0, n), kinds, "environment 3"),
                                   (np.where(np.arange(24) == 20, 9, n), kinds, "environment 20"),
                                   (n, np.where(absent_mask(scs, 8) & (np.arange(24) == 9)[:, None] & (np.arange(8) == 6), 2, kinds),
                                    "environment 9, body 6")):
            with pytest.raises(rb.RbError, match=what) as ei:
                b.set_population(bad_n, bad_k)
            assert ei.value.code == EINVAL
        with pytest.raises(rb.RbError) as ei:
            b.set_contact_law("balls")
        assert ei.value.code == EUNSUPPORTED
        got_n, got_k = b.population
        assert np.array_equal(got_n, n) and np.array_equal(got_k, kinds)
        assert b.step(20) == 0
        got = b.get_state()
    assert _same(got[0], want[0]) and _same(got[1], want[1])


def test_set_population_is_refused_under_the_two_ball_law(rb, oracle):
    """RB_EUNSUPPORTED, after which the uniform batch steps as one that never saw the call."""
    from rbhip import scenes
    sc = scenes.flat_spheres(2, 2, seed=3, spacing=0.19)
    with rb.BatchWorld(sc, 5, law="balls") as a:
        assert a.step(20) == 0
        want = a.get_state()
    with rb.BatchWorld(sc, 5, law="balls") as b:
        with pytest.raises(rb.RbError) as ei:
            b.set_population(np.array([1, 2, 3, 4, 4]), None)
        assert ei.value.code == EUNSUPPORTED and b.population is None
        assert b.step(20) == 0
        got = b.get_state()
    assert _same(got[0], want[0]) and _same(got[1], want[1])
