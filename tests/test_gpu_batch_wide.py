"""Wide batches (rb_batch_create_wide; batch_wide_kernel and
wide_contacts_kernel, rb_batch_wide.hip): environments of 65 to 256 bodies,
one per workgroup of 2 to 4 waves.  Every environment steps bit-identically
(uint64 words; no tolerance anywhere) to the committed oracle run on that
environment's own scene with max_partners 64 (a wide environment has no partner
cap; the oracle records at most 8 contacts per body on these scenes), one step
at a time with its contact records read.  Every stepping test asserts from those
records that bodies of different waves touched (partner j of body i with
j // 64 != i // 64), and on box scenes that every box kind (17, 32..35, 40) and
a plane-box corner was recorded, so a run in which the waves never meet cannot
pass.  The contact query is held to the long-double reference of
tests/contact_geometry.py and to the oracle's lists as
test_gpu_contact_geometry.py::test_batch_query holds the one-wave query."""
from collections import Counter

import numpy as np
import pytest

import contact_geometry as cg

pytestmark = pytest.mark.gpu

EDOM = -33
EUNSUPPORTED = -95
BOX_KINDS = (17, 32, 33, 34, 35, 40)


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
    """Bit identity as words of the arrays' own width (the sign of zeros counts)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    w = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(w), b.view(w))


def _differing(q, v, rq, rv):
    return [k for k in range(q.shape[0]) if not (_same(q[k], rq[k]) and _same(v[k], rv[k]))]


def _states(scs):
    return np.stack([sc.qpos0 for sc in scs]), np.stack([sc.qvel0 for sc in scs])


def oracle_run(oracle, scs, q0, v0, steps, dtype="f64", xfrc=None, keep=()):
    """Environment k through the oracle on scs[k] (max_partners 64; xfrc[k] its
    applied forces), one step at a time.  Returns {t: (q, v)} for t in keep and
    for the last step, a Counter of the recorded contact kinds and the number
    of records whose two bodies lie in different waves, over all environments
    and steps."""
    q, v = np.array(q0, np.float64), np.array(v0, np.float64)
    kept = {t: (q.copy(), v.copy()) for t in tuple(keep) + (steps,)}
    kinds, cross = Counter(), 0
    for k, sc in enumerate(scs):
        osc = oracle.OracleScene(sc, max_partners=64)
        xf = None if xfrc is None else xfrc[k]
        qq, vv = q[k], v[k]
        for t in range(1, steps + 1):
            qq, vv, (cnt, par, kin, dis) = oracle.step(osc, qq, vv, 1, dtype=dtype, xfrc=xf, record=True)
            assert cnt.max() <= 64
            body = np.repeat(np.arange(sc.n), cnt)
            cross += int(((par >= 0) & (par // 64 != body // 64)).sum())
            kinds.update(kin.tolist())
            if t in kept:
                kept[t][0][k], kept[t][1][k] = qq, vv
    for a, b in kept.values():
        assert np.isfinite(a).all() and np.isfinite(b).all()
        a.setflags(write=False)
        b.setflags(write=False)
    return kept, kinds, cross


def _assert_box_kinds(kinds):
    """Every box-involved kind and a plane-box corner were recorded."""
    missing = [c for c in BOX_KINDS if kinds[c] == 0]
    assert not missing and sum(kinds[c] for c in range(1, 9)) > 0, (missing, kinds)


_cache = {}


def _once(key, build):
    """A reference computed once, shared among the tests, never modified."""
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


# ------------------------------------------------------------ the scenes
# name -> (nx, ny, bodies, environments, steps): mixed_spheres(nx, ny, seed=s, spacing=0.19)
SPHERES = {"M65": (13, 5, 65, 5, 200), "M128": (16, 8, 128, 5, 100), "M129": (43, 3, 129, 5, 100),
           "M256": (16, 16, 256, 3, 200)}
PILE70_KEEP = (7, 150, 200)


def sphere_scenes(name):
    from rbhip import scenes
    nx, ny, M, E, steps = SPHERES[name]
    scs = [scenes.mixed_spheres(nx, ny, seed=s, spacing=0.19) for s in range(E)]
    assert scs[0].n == M
    return scs, steps


def pile_scenes(nx, ny, layers, E):
    """box_pile(nx, ny, layers, seed=s) with a restitution and a friction per environment."""
    from rbhip import scenes
    rng = np.random.default_rng(7000 + nx * ny * layers)
    e, mu = rng.uniform(0.0, 0.5, E), rng.uniform(0.1, 0.9, E)
    return [scenes.box_pile(nx, ny, layers, seed=s).with_(restitution=float(e[s]), friction=float(mu[s]))
            for s in range(E)]


def _pile70(oracle, dtype="f64"):
    """The 70-body piles (E = 5) and their oracle states after 7, 150 and 200
    steps, in fp64 after 300 too."""
    steps = 300 if dtype == "f64" else 200

    def build():
        scs = pile_scenes(4, 4, 4, 5)
        assert scs[0].n == 70 and set(scs[0].kind.tolist()) == {0, 1}
        q0, v0 = _states(scs)
        kept, kinds, cross = oracle_run(oracle, scs, q0, v0, steps, dtype=dtype, keep=PILE70_KEEP)
        return dict(scs=scs, q0=q0, v0=v0, ref=kept, kinds=kinds, cross=cross)
    return _once(("pile70", dtype), build)


def _pile_batch(rb, d, n=None, **kw):
    """The piles d["scs"][:n] as a batch, restitution and friction given through set_params."""
    scs = d["scs"][:n]
    b = rb.BatchWorld.from_scenes([sc.with_(restitution=0.0, friction=0.0) for sc in scs], **kw)
    b.set_params(restitution=[sc.restitution for sc in scs], friction=[sc.friction for sc in scs])
    return b


# ------------------------------------------------------------ 1. spheres across 2, 3 and 4 waves
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", list(SPHERES))
def test_spheres_bit_exact(rb, oracle, name, dtype):
    """M = 65 (one body in the second wave), 128 (two full waves), 129 (one
    body in the third) and 256 (four full waves)."""
    scs, steps = sphere_scenes(name)
    q0, v0 = _states(scs)
    ref, kinds, cross = _once(("spheres", name, dtype), lambda: oracle_run(oracle, scs, q0, v0, steps, dtype=dtype))
    assert cross > 0 and kinds[16] > 0, (cross, kinds)
    with rb.BatchWorld.from_scenes(scs, dtype=dtype) as b:
        assert b.n_bodies == scs[0].n > 64
        assert b.step(steps) == 0
        q, v = b.get_state()
        code, done = b.status()
    bad = _differing(q, v, *ref[steps])
    assert not bad, f"environments differing from the oracle: {bad}"
    assert not code.any() and (done == steps).all()


# ------------------------------------------------------------ 2. mixed bodies
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_pile_of_70_bit_exact(rb, oracle, dtype):
    """box_pile(4, 4, 4): 16 columns of four cubes, six of them with a sphere
    cap, column by column: the last column and its cap lie in the second wave.
    Compared after 7, 150 and 200 steps."""
    d = _pile70(oracle, dtype)
    assert d["cross"] > 0
    _assert_box_kinds(d["kinds"])
    with _pile_batch(rb, d, dtype=dtype) as b:
        at = 0
        for t in PILE70_KEEP:
            assert b.step(t - at) == 0
            at = t
            q, v = b.get_state()
            bad = _differing(q, v, *d["ref"][t])
            assert not bad, f"after step {t}: environments differing from the oracle: {bad}"


def test_pile_of_214_bit_exact(rb, oracle):
    """box_pile(8, 8, 3): 214 bodies in four waves (block 256 with 42 idle lanes), E = 2, 120 steps."""
    def build():
        scs = pile_scenes(8, 8, 3, 2)
        assert scs[0].n == 214
        q0, v0 = _states(scs)
        return (scs,) + oracle_run(oracle, scs, q0, v0, 120)
    scs, ref, kinds, cross = _once("pile214", build)
    assert cross > 0
    _assert_box_kinds(kinds)
    with _pile_batch(rb, dict(scs=scs)) as b:
        assert b.step(120) == 0
        q, v = b.get_state()
    bad = _differing(q, v, *ref[120])
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ 3. the cut
def test_cut_independence(rb, oracle):
    """300 steps as one call (two launches: 256 + 44), as 256 + 44 and as
    7 + 293 give the same words, the oracle's."""
    d = _pile70(oracle)
    assert d["cross"] > 0
    _assert_box_kinds(d["kinds"])
    got = []
    for cut in ((300,), (256, 44), (7, 293)):
        with _pile_batch(rb, d, 3) as b:
            for n in cut:
                assert b.step(n) == 0
            got.append(b.get_state())
            assert (b.status()[1] == 300).all()
    for q, v in got[1:]:
        assert _same(q, got[0][0]) and _same(v, got[0][1])
    rq, rv = d["ref"][300]
    assert not _differing(got[0][0], got[0][1], rq[:3], rv[:3])


# ------------------------------------------------------------ 4. failure stays per environment
def test_failure_freezes_the_whole_environment_and_no_other(rb, oracle):
    """Body 69 (the second wave) of environment 2 starts outside the domain of
    the position check (|x| / cell >= 2^29, cell = 4 rmax 1.001 < 3 m: 1e12 m
    is out).  The environment keeps its start state in every body, the 64 of
    the first wave included, reports RB_EDOM with no step done, and a reset
    revives it; the other environments step as the oracle does."""
    d = _pile70(oracle)
    assert d["cross"] > 0
    others = [0, 1, 3, 4]
    q0 = d["q0"].copy()
    q0[2, 69, 0] = 1e12
    with _pile_batch(rb, d) as b:
        b.set_state(q0, d["v0"])
        assert b.step(150) == 1
        code, done = b.status()
        q, v = b.get_state()
        assert code[2] == EDOM and done[2] == 0
        assert not code[others].any() and (done[others] == 150).all()
        assert _same(q[2], q0[2]) and _same(v[2], d["v0"][2])
        rq, rv = d["ref"][150]
        assert _same(q[others], rq[others]) and _same(v[others], rv[others])
        b.set_state(d["q0"][[2]], d["v0"][[2]], envs=[2])
        assert b.step(7) == 0
        code, done = b.status()
        assert not code.any() and done[2] == 7 and (done[others] == 157).all()
        q, v = b.get_state(envs=[2])
    assert _same(q[0], d["ref"][7][0][2]) and _same(v[0], d["ref"][7][1][2])


# ------------------------------------------------------------ 5. sampled runs
def test_sampled_runs(rb, torch, oracle):
    """run_sampled(300, 7) and run_sampled_device(300, 7) (the REC instances;
    the second launch starts inside a sampling period) equal the step(7) +
    get_state() loop word for word and end in the state of step(300)."""
    d = _pile70(oracle)
    assert d["cross"] > 0
    E, S = 3, 300 // 7
    with _pile_batch(rb, d, E) as a:
        lq, lv = np.zeros((S, E, 70, 7)), np.zeros((S, E, 70, 6))
        for s in range(S):
            assert a.step(7) == 0
            lq[s], lv[s] = a.get_state()
    assert _same(lq[0], d["ref"][7][0][:E]) and _same(lv[0], d["ref"][7][1][:E])
    with _pile_batch(rb, d, E) as b:
        sq, sv, nf = b.run_sampled(300, 7)
        fq, fv = b.get_state()
    assert nf == 0 and _same(sq, lq) and _same(sv, lv)
    assert _same(fq, d["ref"][300][0][:E]) and _same(fv, d["ref"][300][1][:E])
    with _pile_batch(rb, d, E) as c:
        c.use_stream(torch.cuda.current_stream().cuda_stream)
        dq, dv = c.run_sampled_device(300, 7)
        assert c.sync() == 0
        fq, fv = c.get_state()
    assert _same(dq.cpu().numpy(), lq) and _same(dv.cpu().numpy(), lv)
    assert _same(fq, d["ref"][300][0][:E]) and _same(fv, d["ref"][300][1][:E])


# ------------------------------------------------------------ 6. planes, gravity and forces per environment
def _env_knobs(scs):
    """A ground tilted by up to 0.05 rad about a random horizontal axis,
    gravity (U(-0.3, 0.3), U(-0.3, 0.3), -9.8 U(0.8, 1.2)), and on every body
    a force of m N(0, 1) N and a torque ~ N(0, 1e-3) N m."""
    E, M = len(scs), scs[0].n
    rng = np.random.default_rng(611 + M)
    tilt, az = rng.uniform(0.0, 0.05, E), rng.uniform(0.0, 2 * np.pi, E)
    planes = np.zeros((E, 1, 6))
    planes[:, 0, 0], planes[:, 0, 1], planes[:, 0, 2] = np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)
    gravity = np.stack([rng.uniform(-0.3, 0.3, E), rng.uniform(-0.3, 0.3, E), -9.8 * rng.uniform(0.8, 1.2, E)], axis=1)
    mass = np.stack([sc.mass for sc in scs])
    xfrc = np.concatenate([mass[:, :, None] * rng.normal(0.0, 1.0, (E, M, 3)), rng.normal(0.0, 1e-3, (E, M, 3))], axis=2)
    return planes, gravity, xfrc


@pytest.mark.parametrize("which", ["M65", "pile70"])
def test_per_environment_planes_gravity_forces(rb, oracle, which):
    """The ENVS instances: from_scenes over scenes that differ in gravity and
    planes, then set_xfrc, against the oracle given the same."""
    def build():
        if which == "M65":
            base, steps = sphere_scenes("M65")
        else:
            base, steps = pile_scenes(4, 4, 4, 5), 150
        planes, gravity, xfrc = _env_knobs(base)
        assert np.abs(xfrc).min() > 0
        scs = [sc.with_(planes=planes[k], gravity=gravity[k]) for k, sc in enumerate(base)]
        q0, v0 = _states(scs)
        return (scs, steps, xfrc) + oracle_run(oracle, scs, q0, v0, steps, xfrc=xfrc)
    scs, steps, xfrc, ref, kinds, cross = _once(("envs", which), build)
    assert cross > 0, kinds
    if which == "pile70":
        _assert_box_kinds(kinds)
    with rb.BatchWorld.from_scenes(scs) as b:
        b.set_xfrc(xfrc)
        assert b.step(steps) == 0
        q, v = b.get_state()
    bad = _differing(q, v, *ref[steps])
    assert not bad, f"environments differing from the oracle: {bad}"


# ------------------------------------------------------------ 7. the device-resident boundary
def test_device_boundary_equals_the_host_forms(rb, torch, oracle):
    """set_state_device with a reset mask, get_state_device, set_xfrc_device
    and status_device on one batch, set_state(envs=...), get_state, set_xfrc
    and status on another: the same words after the same steps."""
    d = _pile70(oracle)
    assert d["cross"] > 0
    E = 5
    dev = lambda a: torch.from_numpy(np.array(a)).to("cuda:0")        # noqa: E731
    rng = np.random.default_rng(77)
    xfrc = np.concatenate([rng.normal(0.0, 0.5, (E, 70, 3)), rng.normal(0.0, 0.05, (E, 70, 3))], axis=2)
    mask = np.array([0, 1, 0, 1, 0], np.uint8)
    ids = [1, 3]
    with _pile_batch(rb, d) as h, _pile_batch(rb, d) as g:
        g.use_stream(torch.cuda.current_stream().cuda_stream)
        h.set_xfrc(xfrc)
        g.set_xfrc_device(dev(xfrc))
        assert h.step(20) == 0
        g.step_async(20)
        # a reset of environments 1 and 3 (the rows of the others are not read)
        h.set_state(d["q0"][ids], d["v0"][ids], envs=ids)
        up_q, up_v = np.full((E, 70, 7), np.nan), np.full((E, 70, 6), np.nan)
        up_q[ids], up_v[ids] = d["q0"][ids], d["v0"][ids]
        g.set_state_device(dev(up_q), dev(up_v), mask=dev(mask))
        assert h.step(13) == 0
        g.step_async(13)
        gq, gv = g.get_state_device()
        gcode, gdone = g.status_device()
        assert g.sync() == 0
        hq, hv = h.get_state()
        hcode, hdone = h.status()
        assert _same(gq.cpu().numpy(), hq) and _same(gv.cpu().numpy(), hv)
        assert np.array_equal(gcode.cpu().numpy(), hcode) and np.array_equal(gdone.cpu().numpy(), hdone)
        assert hdone.tolist() == [33, 13, 33, 13, 33]
        q2, v2 = g.get_state()
        assert _same(q2, hq) and _same(v2, hv)
    # and the host form is the oracle's: environments 1 and 3, 13 steps from the start under their forces
    scs = [d["scs"][k] for k in ids]
    ref, _, _ = oracle_run(oracle, scs, d["q0"][ids], d["v0"][ids], 13, xfrc=xfrc[ids])
    assert _same(hq[ids], ref[13][0]) and _same(hv[ids], ref[13][1])


# ------------------------------------------------------------ 8. the contact query
# family, M, E.  The plane family runs in fp64 only: its bodies lie up to M
# PLANE_SLOT from the point the planes pass through, where the fp32 rounding of
# (c - pp).n is above the fp32 near bound (test_gpu_contact_geometry.py); the
# mixed family is asked for in both real types.
QUERY = [("pairs_random", 66, 5, "f64"), ("pairs_random", 256, 3, "f64"), ("pairs_grazing", 130, 3, "f64"),
         ("plane_random", 65, 5, "f64"), ("mixed", 70, 5, "f64"), ("mixed", 70, 5, "f32"), ("mixed", 200, 2, "f64"),
         ("mixed", 200, 2, "f32")]


def _query_problem(family, M, E, dtype):
    if family == "mixed":
        pb = cg.mixed(E, seed=300 + M, M=M)
        return pb.rounded() if dtype == "f32" else pb
    n = E * M if family in cg.PLANE_FAMILIES else E * (M // 2)
    return cg.make(family, n=n, dtype=dtype, M=M)


@pytest.mark.parametrize("family,M,E,dtype", QUERY, ids=[f"{f}-M{M}-{d}" for f, M, E, d in QUERY])
def test_contact_query(rb, oracle, family, M, E, dtype):
    def build():
        pb = _query_problem(family, M, E, dtype)
        lists = cg.oracle_lists(oracle, pb, dtype)
        for a in lists + (pb.qpos, pb.size, pb.planes):
            a.setflags(write=False)
        return pb, cg.reference_lists(pb), lists
    pb, ref, want = _once(("query", family, M, dtype), build)
    assert pb.M == M > 64 and pb.G == E and want[0].sum() > 0 and want[0].max() <= 16
    if family == "mixed":       # (a pair family's pairs are bodies 2p, 2p + 1: never two waves)
        body = np.repeat(np.arange(pb.N) % M, want[0])
        assert ((want[1] >= 0) & (want[1] // 64 != body // 64)).any(), "no record between bodies of different waves"
    with rb.BatchWorld.from_scenes(pb.scenes(), dtype=dtype) as b:
        b.set_planes(pb.planes)
        b.set_state(pb.qpos.reshape(pb.G, pb.M, 7), np.zeros((pb.G, pb.M, 6)))
        con = b.contacts(max_records=16)
        assert con.truncated == 0
        got = cg.dense_lists(con)
    cg.assert_properties(got, pb, dtype, ref)
    bad = []
    for name, g, w in zip(("counts", "partner", "kind", "dist", "pos", "frame"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        # word for word in fp64; the same values in fp32 (both sides hold floats widened to double)
        if g.shape != w.shape or not (_same(g, w) if g.dtype.kind == "f" and dtype == "f64" else np.array_equal(g, w)):
            bad.append(name)
    assert not bad


# ------------------------------------------------------------ 9, 10. below the line; refusals
class _WideEntry:
    """The library with rb_batch_create and rb_batch_create_mixed answered by
    rb_batch_create_wide: BatchWorld picks that entry by itself only above 64 bodies."""

    def __init__(self, L):
        self._L = L

    def __getattr__(self, name):
        return getattr(self._L, "rb_batch_create_wide" if name in ("rb_batch_create", "rb_batch_create_mixed") else name)


@pytest.fixture
def wide_entry(rb, monkeypatch):
    from rbhip import _lib
    real = _lib.load()
    monkeypatch.setattr(_lib, "load", lambda *a, **k: _WideEntry(real))


def test_below_the_line_equals_create_mixed(rb, oracle, monkeypatch):
    """A 14-body pile through rb_batch_create_wide is the batch
    rb_batch_create_mixed gives: the same words after 200 steps."""
    from rbhip import scenes, _lib
    scs = [scenes.box_pile(2, 2, 3, seed=s) for s in range(9)]
    assert scs[0].n == 14
    with rb.BatchWorld.from_scenes(scs) as b:
        assert b.step(200) == 0
        mq, mv = b.get_state()
    real = _lib.load()
    calls = []

    class Spy(_WideEntry):
        def __getattr__(self, name):
            calls.append(name)
            return _WideEntry.__getattr__(self, name)
    monkeypatch.setattr(_lib, "load", lambda *a, **k: Spy(real))
    with rb.BatchWorld.from_scenes(scs) as b:
        assert b.step(200) == 0
        wq, wv = b.get_state()
    assert "rb_batch_create_mixed" in calls          # (answered by rb_batch_create_wide)
    assert _same(wq, mq) and _same(wv, mv)
    ref, kinds, _ = oracle_run(oracle, scs[:2], *(a[:2] for a in _states(scs)), 200)
    _assert_box_kinds(kinds)
    assert _same(wq[:2], ref[200][0]) and _same(wv[:2], ref[200][1])


def test_two_ball_law_is_refused_above_64(rb, oracle, wide_entry):
    """RB_EUNSUPPORTED on a 65-sphere wide batch, at construction and from
    set_contact_law, after which the batch steps as before; accepted on a
    64-sphere batch made by the same entry."""
    from rbhip import scenes
    scs, _ = sphere_scenes("M65")
    sc = scs[0].with_(planes=np.array([[0.0, 0, 1, 0, 0, 0]]))
    with pytest.raises(rb.RbError) as ei:
        rb.BatchWorld(sc, 2, law="balls")
    assert ei.value.code == EUNSUPPORTED
    ref, _, _ = oracle_run(oracle, [sc], sc.qpos0[None], sc.qvel0[None], 7)
    with rb.BatchWorld(sc, 2) as b:
        with pytest.raises(rb.RbError, match="64") as ei:
            b.set_contact_law("balls")
        assert ei.value.code == EUNSUPPORTED
        assert b.step(7) == 0
        q, v = b.get_state()
    assert _same(q[0], ref[7][0][0]) and _same(q[1], ref[7][0][0]) and _same(v[0], ref[7][1][0])
    s64 = scenes.balls_pile(8, 8)
    assert s64.n == 64
    with rb.BatchWorld(s64, 2) as b:
        b.set_contact_law("balls")
        assert b.step(7) == 0
