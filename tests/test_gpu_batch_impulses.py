"""The impulse query of a batch (rb_batch_impulses, rb_batch_impulses_dev;
BatchWorld.impulses / impulses_device; kernels in rb_batch_impulses.hip).

1. Against the CPU model (tests/impulse_model.py, itself held to the oracle's
   step by tests/test_impulse_model.py): every word of counts, partner, kind,
   dist, jn, jt, vel and net, per environment, f64 and f32.
2. Against the step, bit for bit, no model: imp.vel equals the qvel that the
   next step(1) writes, for every mapping and instance.
3. Against the contact query: counts, partner, kind, dist word for word.
4. Truncation drops records only.  5. The parameters of the call count.
6. The query changes nothing.  7. Failed environments and absent bodies.
8. The device form.  9. Refusals.  The host form's cut into launches.

Shapes are the smallest that reach each kernel instance: M = 1, 4 (one wave,
idle lanes in the last wave at E = 7), 70 (128 threads), 144 (192 threads), a
population of 1..8 bodies; E between 2 and 24."""
import numpy as np
import pytest

import impulse_model as IM

pytestmark = pytest.mark.gpu

EINVAL = -22
EDOM = -33
EUNSUPPORTED = -95
RECORDS = ("counts", "partner", "kind", "dist")
FIELDS = ("counts", "partner", "kind", "dist", "jn", "jt", "vel", "net")
REALS = ("dist", "jn", "jt", "vel", "net")


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


def _w(a):
    """The words of an array (reals as uint64: the sign of zeros counts)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_w(a), _w(b))


def differing(imp, ref, fields=FIELDS, rows=None):
    """The fields of imp (a BatchImpulses, or a mapping) that differ from ref's in any word."""
    get = (lambda o, f: o[f]) if isinstance(imp, dict) else getattr
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    return [f for f in fields if not _same(pick(np.asarray(get(imp, f))), np.asarray(ref[f]))]


def model_dense(scs, q, v, R, dtype="f64", **params):
    """The model of every environment k (scene scs[k], state q[k], v[k]) in the
    query's dense layout, and the branch counts summed."""
    out = {f: [] for f in FIELDS}
    stats = dict(applied=0, separating=0, skipped=0)
    for k, sc in enumerate(scs):
        m = IM.impulses(sc, q[k], v[k], dtype=dtype, max_partners=32, **params)
        counts, partner, kind, dist, jn, jt = IM.dense(m, R)
        for f, a in zip(FIELDS, (counts, partner, kind, dist, jn, jt, m.vel, m.net)):
            out[f].append(a)
        for s in stats:
            stats[s] += getattr(m, s)
    return {f: np.stack(a) for f, a in out.items()}, stats


def box_sweep():
    """A friction sweep of box_pile(1, 1, 3): three cubes and a sphere, 5 environments."""
    from rbhip import scenes
    return [scenes.box_pile(1, 1, 3).with_(friction=f) for f in (0.0, 0.2, 0.5, 0.8, 1.2)]


def sphere_sweep():
    """multi_sphere4 with a restitution per environment, 7 environments (M = 4:
    16 per wave, so one wave with idle lanes)."""
    from rbhip import scenes
    return [scenes.multi_sphere4().with_(restitution=float(e)) for e in np.linspace(0.2, 0.95, 7)]


# ------------------------------------------------------------ 1. against the model
# The box pile is in contact from step 0 on.  The spheres fall for 62 steps: the
# first query step is the step of the first impact (all environments), not 0,
# where the oracle holds no contact at all; 100 and 300 hold bounces of the
# environments with low restitution.
SWEEPS = {"boxes": (box_sweep, (0, 40, 120)), "spheres": (sphere_sweep, (62, 100, 300))}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("which", list(SWEEPS))
def test_every_word_equals_the_model(rb, oracle, which, dtype):
    make, steps = SWEEPS[which]
    scs = make()
    with rb.BatchWorld.from_scenes(scs, dtype=dtype) as b:
        R = b._max_records(None)
        done = 0
        for t in steps:
            assert b.step(t - done) == 0
            done = t
            q, v = b.get_state()
            imp = b.impulses()
            ref, stats = model_dense(scs, q, v, R, dtype=dtype)
            print(f"{which} {dtype} step {t}: {int(ref['counts'].sum())} records, {stats}")
            assert (ref["jn"] != 0).any() and stats["applied"] > 0, t          # (checked on the CPU first)
            assert not differing(imp, ref), t
            assert imp.truncated == int((ref["counts"] > R).sum())
            assert imp.partner.shape == (len(scs), scs[0].n, R) and imp.jt.shape == (len(scs), scs[0].n, R, 3)


# ------------------------------------------------------------ 2. against the step
def ragged_scenes():
    """The 24-environment population of 1 to 8 bodies of tests/test_gpu_batch_ragged.py
    (its ensemble 1): more than ten kind patterns, M = 8, 87 present bodies."""
    from rbhip import scenes
    return [scenes.box_pile(1 + (s // 3) % 2, 1, 1 + s % 3, seed=s, sphere_every=(0, 1, 3)[(s // 6) % 3])
            for s in range(24)]


def _make_case(rb, name):
    """(batch, present (E, M) bool, steps to run before the first query)"""
    from rbhip import scenes
    if name == "single_cube":                            # M = 1: the one-box path of the plain instance
        scs = [scenes.single_cube().with_(friction=f) for f in (0.1, 0.5, 0.9)]
        return rb.BatchWorld.from_scenes(scs), np.ones((3, 1), bool), 0
    if name == "multi_sphere4":                          # E = 7: idle lanes in the last wave; first impact at step 62
        return rb.BatchWorld.from_scenes(sphere_sweep()), np.ones((7, 4), bool), 62
    if name == "box_pile_1_1_3":                         # mixed, one wave
        return rb.BatchWorld.from_scenes(box_sweep()), np.ones((5, 4), bool), 0
    if name == "box_pile_4_4_4":                         # 70 bodies: 128 threads, boxes
        b = rb.BatchWorld(scenes.box_pile(4, 4, 4), 2)
        b.set_params(friction=[0.2, 0.9])
        return b, np.ones((2, 70), bool), 0
    if name == "flat_spheres_12_12":                     # 144 bodies: 192 threads, spheres
        b = rb.BatchWorld(scenes.flat_spheres(12, 12, spacing=0.19), 2)
        b.set_params(restitution=[0.3, 0.8])
        return b, np.ones((2, 144), bool), 0
    if name == "population":
        scs = ragged_scenes()
        n = np.array([sc.n for sc in scs])
        assert sorted(set(n)) == list(range(1, 9)) and n.sum() == 87
        return rb.BatchWorld.from_ragged_scenes(scs), np.arange(8)[None, :] < n[:, None], 0
    if name == "population_of_one":                      # M = 1 with kinds per environment: the box instance at M = 1
        cube = scenes.single_cube()
        scs = [cube, scenes.single_sphere().with_(dt=cube.dt, threshold=cube.threshold)] * 3
        return rb.BatchWorld.from_ragged_scenes(scs), np.ones((6, 1), bool), 0
    assert name == "planes_gravity_forces"
    scs = box_sweep()
    E, M = len(scs), scs[0].n
    b = rb.BatchWorld.from_scenes(scs)
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


CASES = ["single_cube", "multi_sphere4", "box_pile_1_1_3", "box_pile_4_4_4", "flat_spheres_12_12", "population",
         "population_of_one", "planes_gravity_forces"]


@pytest.mark.parametrize("name", CASES)
def test_vel_is_the_qvel_of_the_next_step(rb, name):
    b, present, pre = _make_case(rb, name)
    with b:
        assert b.step(pre) == 0
        nonzero = contacts = 0
        for t in range(60):
            if t % 10:
                b.step(1)
                continue
            imp = b.impulses()
            b.step(1)
            _, v = b.get_state()
            code, _ = b.status()
            ok = (code == 0)[:, None] & present
            assert ok.any()
            assert np.array_equal(_w(imp.vel)[ok], _w(v)[ok]), (name, t)
            assert (imp.counts[~present] == 0).all() and not _w(imp.vel)[~present].any()
            nonzero += int((imp.jn != 0).sum())
            contacts += int(np.maximum(imp.counts, 0).sum())
        assert not b.status()[0].any()
    print(f"{name}: {contacts} contacts, {nonzero} with jn != 0 over the six queries")
    assert nonzero > 0


# ------------------------------------------------------------ 3, 4. the contact query; truncation
@pytest.fixture(scope="module")
def pile120(rb):
    """The box sweep at step 120 (up to 8 records per body): its batch, open for the module."""
    scs = box_sweep()
    b = rb.BatchWorld.from_scenes(scs)
    assert b.step(120) == 0
    yield scs, b
    b.close()


@pytest.mark.parametrize("R", [1, 4, None])
def test_records_equal_the_contact_query(pile120, R):
    _, b = pile120
    imp, con = b.impulses(max_records=R), b.contacts(max_records=R)
    assert imp.counts.max() > 4 and imp.partner.shape == con.partner.shape
    assert not differing(imp, {f: getattr(con, f) for f in RECORDS}, RECORDS)
    assert imp.truncated == con.truncated == int((con.counts > imp.partner.shape[-1]).sum())
    assert imp.truncated > 0 or R is None


def test_truncation_drops_records_only(pile120):
    _, b = pile120
    full, one, none = b.impulses(), b.impulses(max_records=1), b.impulses(max_records=0)
    assert none.partner is None and none.jn is None and none.jt is None and none.truncated == int((full.counts > 0).sum())
    assert one.truncated == int((full.counts > 1).sum()) > 0 and full.truncated == 0
    for q in (one, none):
        assert not differing(q, {f: getattr(full, f) for f in ("counts", "vel", "net")}, ("counts", "vel", "net"))
    assert full.net.any() and _same(one.jn, full.jn[:, :, :1]) and _same(one.jt, full.jt[:, :, :1])


def test_host_form_is_cut_into_launches(rb, pile120, monkeypatch):
    """The staging buffer (RBHIP_BATCH_SAMPLE_BYTES, read at creation) sized for
    two environments: five listed environments, out of order, take three
    launches and give the rows of the uncut query; one byte short of one
    environment is RB_EINVAL."""
    scs, whole = pile120
    M, R = scs[0].n, 8
    per = 8 * (5 * M * R + 12 * M) + 4 * (M + 2 * M * R)       # reals first, then the words
    order = [4, 0, 2, 3, 1]
    ref = whole.impulses(envs=order, max_records=R)
    assert not differing(ref, {f: getattr(whole.impulses(max_records=R), f)[order] for f in FIELDS})
    q, v = whole.get_state()
    monkeypatch.setenv("RBHIP_BATCH_SAMPLE_BYTES", str(2 * per))
    with rb.BatchWorld.from_scenes(scs) as b:
        b.set_state(q, v)
        cut = b.impulses(envs=order, max_records=R)
        assert not differing(cut, {f: getattr(ref, f) for f in FIELDS}) and cut.truncated == ref.truncated
    monkeypatch.setenv("RBHIP_BATCH_SAMPLE_BYTES", str(per - 1))
    with rb.BatchWorld.from_scenes(scs) as b:
        b.set_state(q, v)
        with pytest.raises(rb.RbError) as ei:
            b.impulses(max_records=R)
        assert ei.value.code == EINVAL
        assert b.impulses(max_records=0).counts.shape == (5, M)          # (the sensor-only rows fit)


# ------------------------------------------------------------ 5. the parameters count
def test_parameters_of_the_call_count(rb, pile120):
    scs, b = pile120
    q, v = b.get_state()
    R = b._max_records(None)
    base = b.impulses()
    dt, e = scs[0].dt, scs[0].restitution
    # (from_scenes set per-environment restitution and friction: the scalars of a call do not reach the law)
    assert not differing(b.impulses(restitution=0.9, friction=0.05), {f: getattr(base, f) for f in FIELDS})
    twice = b.impulses(dt=2 * dt)
    assert "vel" in differing(twice, {f: getattr(base, f) for f in FIELDS})
    assert not differing(twice, model_dense(scs, q, v, R, dt=2 * dt)[0])
    strict = b.impulses(threshold=0.002)
    ref, stats = model_dense(scs, q, v, R, threshold=0.002)
    assert stats["skipped"] > 0 and not differing(strict, ref) and "jn" in differing(strict, {f: getattr(base, f) for f in FIELDS})
    # scalars alone: a batch without per-environment values
    with rb.BatchWorld(scs[2], 3) as c:
        q3, v3 = np.stack([q[2]] * 3), np.stack([v[2]] * 3)
        c.set_state(q3, v3)
        plain, bouncy = c.impulses(), c.impulses(restitution=0.9)
        assert "jn" in differing(bouncy, {f: getattr(plain, f) for f in FIELDS})
        assert not differing(bouncy, model_dense([scs[2].with_(restitution=0.9)] * 3, q3, v3, R)[0])
        assert not differing(plain, {f: getattr(base, f)[[2, 2, 2]] for f in FIELDS})
        # set_params takes precedence over the scalars
        c.set_params(restitution=[e, 0.9, e])
        mixed = c.impulses(restitution=0.5)
        assert not differing(mixed, {f: np.stack([getattr(plain, f)[0], getattr(bouncy, f)[1], getattr(plain, f)[2]])
                                     for f in FIELDS})


# ------------------------------------------------------------ 6. the query changes nothing
def test_query_changes_nothing(rb):
    scs = box_sweep()
    with rb.BatchWorld.from_scenes(scs) as a, rb.BatchWorld.from_scenes(scs) as b:
        seen = 0
        for chunk in (40, 60, 30, 70):
            assert a.step(chunk) == 0 and b.step(chunk) == 0
            host = a.impulses()
            dev = a.impulses_device()
            sensor = a.impulses(max_records=0)
            assert a.sync() == 0
            assert np.array_equal(dev.counts.cpu().numpy(), host.counts) and _same(sensor.net, host.net)
            seen += int((host.jn != 0).sum())
        assert seen > 0
        sa, sb = a.get_state(), b.get_state()
        assert all(_same(x, y) for x, y in zip(sa, sb))
        (ca, da), (cb, db) = a.status(), b.status()
        assert np.array_equal(ca, cb) and np.array_equal(da, db) and (da == 200).all()


# ------------------------------------------------------------ 7. failure and absence
def test_failed_environment_and_its_neighbours(rb):
    scs = box_sweep()
    with rb.BatchWorld.from_scenes(scs) as b, rb.BatchWorld.from_scenes(scs) as clean:
        assert b.step(40) == 0 and clean.step(40) == 0
        q, v = b.get_state()
        q[3, 1, 2] = np.nan
        b.set_state(q[3:4], v[3:4], envs=[3])
        assert b.step(1) == 1 and clean.step(1) == 0
        code, _ = b.status()
        assert code.tolist() == [0, 0, 0, EDOM, 0]
        imp, ref = b.impulses(), clean.impulses()
        sensor = b.impulses(max_records=0)
    assert (imp.counts[3] == -1).all() and (imp.kind[3] == -1).all() and not imp.partner[3].any()
    assert not any(_w(getattr(imp, f)[3]).any() for f in REALS)
    assert (sensor.counts[3] == -1).all() and not _w(sensor.vel[3]).any() and not _w(sensor.net[3]).any()
    others = [0, 1, 2, 4]
    assert (ref.jn[others] != 0).any()
    assert not differing(imp, {f: getattr(ref, f)[others] for f in FIELDS}, rows=others)
    assert imp.truncated == ref.truncated


def test_absent_bodies(rb):
    scs = ragged_scenes()
    n = np.array([sc.n for sc in scs])
    absent = np.arange(8)[None, :] >= n[:, None]
    with rb.BatchWorld.from_ragged_scenes(scs) as b:
        assert b.step(30) == 0
        imp = b.impulses(max_records=8)
        assert (imp.counts[absent] == 0).all() and (imp.kind[absent] == -1).all() and not imp.partner[absent].any()
        assert not any(_w(getattr(imp, f))[absent].any() for f in REALS)
        assert (imp.jn != 0).any() and (imp.partner[imp.kind >= 0] < n[np.nonzero(imp.kind >= 0)[0]]).all()
        # a NaN in an absent slot's state changes nothing
        q, v = b.get_state()
        q[absent], v[absent] = np.nan, np.nan
        b.set_state(q, v)
        again = b.impulses(max_records=8)
        assert not b.status()[0].any()
    assert not differing(again, {f: getattr(imp, f) for f in FIELDS})


# ------------------------------------------------------------ 8. the device form
def test_device_form(rb, pile120):
    """impulses_device on a stream of the caller: f64 and f32 element types, new
    tensors and preallocated ones, the sensor-only call."""
    import torch
    scs, b = pile120
    E, M, R = len(scs), scs[0].n, 8
    host = b.impulses(max_records=R)
    stream = torch.cuda.Stream()
    b.use_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            ints = [torch.full(s, 77, dtype=torch.int32, device="cuda") for s in ((E, M), (E, M, R), (E, M, R))]
            reals = [torch.full(s, 7.0, dtype=torch.float32, device="cuda")
                     for s in ((E, M, R), (E, M, R), (E, M, R, 3), (E, M, 6), (E, M, 6))]
            pre = rb.BatchImpulses(*ints, *reals, None)
            ptrs = [getattr(pre, f).data_ptr() for f in FIELDS]
            d64 = b.impulses_device(max_records=R)
            d32 = b.impulses_device(out=pre)
            sensor = b.impulses_device(max_records=0, dtype="f32")
        assert b.sync() == 0
    finally:
        b.use_stream(None)
    assert d64.truncated is None and d64.jn.dtype == torch.float64 and d64.jt.shape == (E, M, R, 3)
    assert not differing({f: getattr(d64, f).cpu().numpy() for f in FIELDS}, {f: getattr(host, f) for f in FIELDS})
    assert d32.counts is pre.counts and d32.net is pre.net and [getattr(pre, f).data_ptr() for f in FIELDS] == ptrs
    for f in FIELDS:
        got, want = getattr(d32, f).cpu().numpy(), getattr(host, f)
        assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32) if f in REALS
                              else want.view(np.uint32)), f
    assert sensor.partner is None and sensor.jn is None and sensor.net.dtype == torch.float32
    assert np.array_equal(sensor.counts.cpu().numpy(), host.counts)
    assert np.array_equal(sensor.vel.cpu().numpy().view(np.uint32), host.vel.astype(np.float32).view(np.uint32))


# ------------------------------------------------------------ 9. refusals on a live batch
def test_refusals_on_a_live_batch(rb):
    from rbhip import _lib, scenes
    sc = scenes.ball_collision()
    with rb.BatchWorld(sc, 3, law="balls") as b:
        for call in (b.impulses, lambda: b.impulses_device(max_records=2)):
            with pytest.raises(rb.RbError) as ei:
                call()
            assert ei.value.code == EUNSUPPORTED
        assert b.step(20) == 0
        b.set_contact_law("mujoco")
        assert b.impulses().counts.shape == (3, 2)
    sc = scenes.multi_sphere4()
    inf, nan = float("inf"), float("nan")
    with rb.BatchWorld(sc, 5) as b:
        assert b.step(62) == 0
        before = b.get_state()
        L, h = b._L, b._h
        cnt, rec = np.full((5, 4), 99, np.int32), np.full((5, 4, 2), 99, np.int32)
        dis, vec, six = np.full((5, 4, 2), 9.0), np.full((5, 4, 2, 3), 9.0), np.full((5, 4, 6), 9.0)
        c, r, d, j3, s6 = (_lib.ptr(a) for a in (cnt, rec, dis, vec, six))
        ids = lambda *a: _lib.ptr(np.array(a, np.int64))     # noqa: E731
        P = (0.01, 0.5, 0.5, 0.0)
        out = (c, r, r, d, d, j3, s6, s6, None)
        refused = [(None, 5, -1, *P, *out),                                    # max_records < 0
                   (None, 5, 0, *P, *out),                                     # max_records 0 with record arrays
                   (None, 5, 2, *P, c, None, None, None, None, None, s6, s6, None),
                   (None, 5, 2, *P, c, r, None, d, d, j3, s6, s6, None),       # not all together
                   (None, 5, 2, *P, c, r, r, d, None, j3, s6, s6, None),       # jn missing
                   (None, 5, 2, *P, c, r, r, d, d, None, s6, s6, None),        # jt missing
                   (None, 5, 0, *P, c, None, None, None, d, j3, s6, s6, None),  # jn, jt with max_records 0
                   (None, 5, 2, *P, None, r, r, d, d, j3, s6, s6, None),       # counts is required
                   (ids(0), -1, 2, *P, *out),                                  # n < 0
                   (None, 4, 2, *P, *out),                                     # all environments: n = n_envs
                   (ids(0, 5), 2, 2, *P, *out),                                # out of range
                   (ids(1, -1), 2, 2, *P, *out),
                   (ids(3, 1, 3), 3, 2, *P, *out)]                             # listed twice
        # the step parameters: what rb_batch_step refuses, and everything non-finite
        for bad in ((0.0, 0.5, 0.5, 0.0), (-0.01, 0.5, 0.5, 0.0), (nan, 0.5, 0.5, 0.0), (inf, 0.5, 0.5, 0.0),
                    (0.01, nan, 0.5, 0.0), (0.01, inf, 0.5, 0.0), (0.01, -0.1, 0.5, 0.0),
                    (0.01, 0.5, nan, 0.0), (0.01, 0.5, inf, 0.0), (0.01, 0.5, -0.1, 0.0),
                    (0.01, 0.5, 0.5, nan), (0.01, 0.5, 0.5, inf), (0.01, 0.5, 0.5, -1.0)):
            if not any(np.isinf(bad)):                                         # (what rb_batch_step refuses too)
                assert L.rb_batch_step(h, 1, *bad, None) == EINVAL, bad
            refused.append((None, 5, 2, *bad, *out))
        for args in refused:
            assert L.rb_batch_impulses(h, *args) == EINVAL, args
        assert (cnt == 99).all() and (rec == 99).all() and (dis == 9.0).all() and (vec == 9.0).all() and (six == 9.0).all()
        # the device form: a host pointer, an unknown element type, the same parameter checks
        assert L.rb_batch_impulses_dev(h, 2, *P, c, r, r, d, d, j3, s6, s6, 0) == EINVAL
        assert b"not device memory" in L.rb_last_error()
        assert L.rb_batch_impulses_dev(h, 2, *P, c, r, r, d, d, j3, s6, s6, 7) == EINVAL
        assert L.rb_batch_impulses_dev(h, 2, nan, 0.5, 0.5, 0.0, c, r, r, d, d, j3, s6, s6, 0) == EINVAL
        assert (cnt == 99).all() and (six == 9.0).all()
        with pytest.raises(TypeError, match="counts"):
            b.impulses_device(out=dict(counts=cnt, partner=None))
        # nothing changed, nothing enqueued: the state, the status, and the next query
        after = b.get_state()
        assert all(_same(x, y) for x, y in zip(before, after))
        code, done = b.status()
        assert not code.any() and (done == 62).all()
        imp = b.impulses(max_records=2)
        assert imp.counts.shape == (5, 4) and (imp.jn != 0).any()
        assert b.step(10) == 0
