"""The contact query of a batch (BatchWorld.contacts / contacts_device;
rb_batch_contacts.hip): for the batch's current state, every environment's
contact lists equal, with no tolerance, what the committed oracle generates
for that environment's scene and state (oracle.contacts with max_partners 32,
its hard limit): counts, partner and kind as integers, dist, pos and frame as
64-bit words, every unused slot's fill included.  The batch's state is read
with get_state() and handed to the oracle, so nothing here depends on how the
state came about.  Every comparison also asserts that the oracle's lists hold
the contact kinds the test is about (0 plane-sphere, 1..8 plane-box corner, 16
sphere-sphere, 17 sphere-box, 32..35 the points of a clipped box-box face, 40
box-box edge-edge): a state in free flight cannot pass.  The floors were
checked on the CPU with the oracle and are weaker than what it lists."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EINVAL, EDOM, EUNSUPPORTED = -22, -33, -95
BOX_KINDS = (17, 32, 33, 34, 35, 40)
FLOAT_FIELDS = ("dist", "pos", "frame")
FIELDS = ("counts", "partner", "kind") + FLOAT_FIELDS


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


def _words(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def dense(lists, M, R):
    """oracle.contacts()' CSR lists of one environment in the query's dense
    layout: the first R records of each body, kind -1 and zeros past them."""
    cnt, par, kin, dis, pos, frm = lists
    out = dict(counts=cnt.astype(np.int32), partner=np.zeros((M, R), np.int32), kind=np.full((M, R), -1, np.int32),
               dist=np.zeros((M, R)), pos=np.zeros((M, R, 3)), frame=np.zeros((M, R, 3)))
    at = 0
    for b in range(M):
        k = min(int(cnt[b]), R)
        for name, src in (("partner", par), ("kind", kin), ("dist", dis), ("pos", pos), ("frame", frm)):
            out[name][b, :k] = src[at:at + k]
        at += int(cnt[b])
    return out


def oracle_dense(oracle, scs, q, R, dtype="f64", max_partners=32):
    """Every environment's oracle lists for the state q (E, M, 7), dense, and
    a Counter of the kinds listed (all records, the ones past R included)."""
    M = q.shape[1]
    per, kinds = [], Counter()
    for k, sc in enumerate(scs):
        lists = oracle.contacts(oracle.OracleScene(sc, max_partners=max_partners), q[k], dtype=dtype)
        kinds.update(lists[2].tolist())
        per.append(dense(lists, M, R))
    return {name: np.stack([p[name] for p in per]) for name in FIELDS}, kinds


def differing(con, ref, got_rows=None, ref_rows=None, exact_words=True, geometry=True):
    """The fields of the query's result that differ from the oracle's dense
    lists (got_rows / ref_rows: the rows of either side to compare)."""
    bad = []
    for name in FIELDS:
        got = getattr(con, name)
        if name in ("pos", "frame") and not geometry:
            assert got is None
            continue
        got, want = np.asarray(got), ref[name]
        got = got if got_rows is None else got[got_rows]
        want = want if ref_rows is None else want[ref_rows]
        if name in FLOAT_FIELDS and exact_words:
            same = got.shape == want.shape and np.array_equal(_words(got), _words(want))
        else:
            same = got.dtype == want.dtype and np.array_equal(got, want)
        if not same:
            bad.append(name)
    return bad


def corners(kinds):
    return sum(kinds[c] for c in range(1, 9))


def assert_box_floors(kinds, each, corner):
    low = {c: kinds[c] for c in BOX_KINDS if kinds[c] < each}
    assert not low and corners(kinds) >= corner, (low, corners(kinds))


# ------------------------------------------------------------ the shapes
E_COL = 37           # M = 4, 16 environments per wave: two full waves and a part
E_RAG = 9            # M = 14, 4 environments per wave and 8 idle lanes
COL_STEPS = (150, 263, 300)


def column_scenes():
    """box_pile(1, 1, 3, seed=s) with the restitution and friction per
    environment of test_gpu_batch_boxes.py."""
    from rbhip import scenes
    rng = np.random.default_rng(1133)
    e, mu = rng.uniform(0.0, 0.5, E_COL), rng.uniform(0.1, 0.9, E_COL)
    return [scenes.box_pile(1, 1, 3, seed=s).with_(restitution=float(e[s]), friction=float(mu[s])) for s in range(E_COL)]


@pytest.fixture(scope="module")
def column(rb, oracle):
    """The column sweep after 150, 263 and 300 steps: the state, the query's
    result (R = 8, geometry) and the oracle's lists (computed once, never
    modified)."""
    scs = column_scenes()
    assert scs[0].n == 4 and list(scs[0].kind) == [1, 1, 1, 0]
    at, done = {}, 0
    with rb.BatchWorld.from_scenes(scs) as b:
        for t in COL_STEPS:
            assert b.step(t - done) == 0
            done = t
            q, _ = b.get_state()
            con = b.contacts(max_records=8)
            ref, kinds = oracle_dense(oracle, scs, q, 8)
            for a in list(ref.values()) + [q] + [getattr(con, f) for f in FIELDS]:
                a.setflags(write=False)
            at[t] = dict(q=q, con=con, ref=ref, kinds=kinds)
    return dict(scs=scs, at=at)


# ------------------------------------------------------------ 1. columns
@pytest.mark.parametrize("t", COL_STEPS)
def test_columns(column, t):
    """M = 4, E = 37.  The oracle lists 38 / 58 / 50 / 36 / 30 / 34 records of
    kinds 17 / 32 / 33 / 34 / 35 / 40 and 56 corners at step 150; 42 / 78 / 76
    / 68 / 52 / 26 and 79 at 263."""
    d = column["at"][t]
    assert_box_floors(d["kinds"], 10, 30)
    assert d["ref"]["counts"].max() == 8
    con = d["con"]
    assert con.max_records == 8 and con.truncated == 0
    assert con.counts.shape == (E_COL, 4) and con.kind.shape == (E_COL, 4, 8) and con.frame.shape == (E_COL, 4, 8, 3)
    assert not differing(con, d["ref"])
    # every unused slot's fill, stated once without the oracle
    unused = np.arange(8)[None, None, :] >= con.counts[:, :, None]
    assert unused.any() and (con.kind[unused] == -1).all() and (con.kind[~unused] >= 0).all()
    for f in ("partner", "dist", "pos", "frame"):
        assert not _words(getattr(con, f)[unused]).any() if f in FLOAT_FIELDS else not con.partner[unused].any()
    # lists(): the CSR shape of oracle.contacts()
    lists = con.lists(3)
    want = column["scs"][3]
    assert lists[0].sum() == lists[1].shape[0] == lists[4].shape[0] and want.n == lists[0].shape[0]


# ------------------------------------------------------------ 2. ragged waves
def test_ragged_waves(rb, oracle):
    """M = 14, E = 9: 8 idle lanes per wave.  At step 150 the oracle lists 16
    / 78 / 66 / 46 / 30 / 32 records of kinds 17 / 32..35 / 40 and 70 corners."""
    from rbhip import scenes
    scs = [scenes.box_pile(2, 2, 3, seed=s) for s in range(E_RAG)]
    assert scs[0].n == 14
    with rb.BatchWorld.from_scenes(scs) as b:
        for n in (150, 150):
            assert b.step(n) == 0
            q, _ = b.get_state()
            con = b.contacts(max_records=8)
            ref, kinds = oracle_dense(oracle, scs, q, 8)
            assert_box_floors(kinds, 10, 60)
            assert not differing(con, ref)
            assert con.truncated == int((ref["counts"] > 8).sum())


# ------------------------------------------------------------ 3. heterogeneous spheres
def test_heterogeneous_spheres(rb, oracle):
    """M = 48, three planes, a radius per body: plane order, -1 - plane, geom1
    = the lower id with unequal radii.  The oracle lists 60 plane and 66
    sphere-sphere records, up to 5 on one body."""
    from rbhip import scenes
    scs = [scenes.mixed_spheres(8, 6, seed=s) for s in range(3)]
    assert scs[0].n == 48 and scs[0].planes.shape[0] == 3
    with rb.BatchWorld.from_scenes(scs) as b:
        assert b.step(200) == 0
        q, _ = b.get_state()
        con = b.contacts(max_records=8)
    ref, kinds = oracle_dense(oracle, scs, q, 8)
    assert kinds[0] >= 40 and kinds[16] >= 40 and ref["counts"].max() >= 4, (kinds, ref["counts"].max())
    assert len(set(ref["partner"][ref["kind"] == 0].tolist())) >= 2          # more than one plane is touched
    assert not differing(con, ref)


# ------------------------------------------------------------ 4. per-environment planes
def _brick_scenes():
    from rbhip import scenes
    br = scenes.trough_bricks(6, seed=2)
    return [br.with_(kind=br.kind[k:k + 1], mass=br.mass[k:k + 1], inertia=br.inertia[k:k + 1], size=br.size[k:k + 1],
                     qpos0=br.qpos0[k:k + 1], qvel0=br.qvel0[k:k + 1]) for k in range(6)]


def _incline_scenes():
    from rbhip import scenes
    return [scenes.cube_incline(0.1 * k) for k in range(8)]


@pytest.mark.parametrize("make,steps", [(_brick_scenes, (60, 40)), (_incline_scenes, (50, 50))],
                         ids=["trough_bricks", "cube_incline"])
def test_per_environment_planes(rb, oracle, make, steps):
    """One-body environments (the one-box instance) with their own planes
    through from_scenes: six bricks in a two-plane trough at steps 60 and 100,
    eight incline angles at steps 50 and 100.  At each of them the oracle
    lists a corner contact in at least half of the environments."""
    scs = make()
    assert scs[0].n == 1 and len({sc.planes.tobytes() for sc in scs}) in (1, len(scs))
    with rb.BatchWorld.from_scenes(scs) as b:
        for n in steps:
            assert b.step(n) == 0
            q, _ = b.get_state()
            con = b.contacts()
            assert con.max_records == 4 * scs[0].planes.shape[0]
            ref, kinds = oracle_dense(oracle, scs, q, con.max_records)
            touching = int((ref["counts"][:, 0] > 0).sum())
            assert 2 * touching >= len(scs) and corners(kinds) == sum(kinds.values()) > 0, (touching, kinds)
            assert not differing(con, ref)


# ------------------------------------------------------------ 5. truncation
def test_truncation(rb, oracle, column):
    d = column["at"][263]
    ref4, _ = oracle_dense(oracle, column["scs"], d["q"], 4)
    assert ref4["counts"].max() == 8
    with rb.BatchWorld.from_scenes(column["scs"]) as b:
        b.set_state(d["q"], np.zeros((E_COL, 4, 6)))
        con = b.contacts(max_records=4)
    assert not differing(con, ref4)
    assert np.array_equal(con.counts, d["con"].counts) and con.counts.max() == 8
    assert np.array_equal(con.kind, d["con"].kind[:, :, :4]) and np.array_equal(_words(con.pos), _words(d["con"].pos[:, :, :4]))
    assert con.truncated == int((ref4["counts"] > 4).sum()) > 0


# ------------------------------------------------------------ 6. counts only, 7. environment lists
def test_counts_only_and_environment_lists(rb, column):
    d = column["at"][263]
    with rb.BatchWorld.from_scenes(column["scs"]) as b:
        b.set_state(d["q"], np.zeros((E_COL, 4, 6)))
        only = b.contacts(max_records=0)
        assert only.partner is None and only.dist is None and only.pos is None and only.truncated == int((d["ref"]["counts"] > 0).sum())
        assert only.counts.dtype == np.int32 and np.array_equal(only.counts, d["ref"]["counts"])
        some = b.contacts(envs=[36, 0, 17], max_records=8)
        assert not differing(some, d["ref"], ref_rows=[36, 0, 17])
        nogeo = b.contacts(envs=[5], max_records=8, geometry=False)
        assert nogeo.pos is None and nogeo.frame is None
        assert not differing(nogeo, {k: v[[5]] for k, v in d["ref"].items()}, geometry=False)


def test_contacts_in_ranges(rb, monkeypatch):
    """The staging buffer (RBHIP_BATCH_SAMPLE_BYTES, read at creation) sized for
    two environments: five environments, listed out of order and all at once,
    take three launches (2, 2, 1) and give every field of the uncut query word
    for word; one byte short of one environment is RB_EINVAL and writes
    nothing.  Five replicas of multi_sphere4 with the balls pressed into the
    ground, each environment to another depth at another place: every
    environment has contacts and no two have the same rows."""
    from rbhip import scenes
    sc = scenes.multi_sphere4()
    E, M, R = 5, sc.n, 4
    # one environment's arrays: counts [M] and partner, kind [M][R] int32; dist [M][R], pos and frame [M][R][3] doubles
    per = 4 * (M + 2 * M * R) + 8 * (M * R + 2 * 3 * M * R)
    q0, v0 = np.tile(sc.qpos0, (E, 1, 1)), np.zeros((E, M, 6))
    q0[:, :, 0] += 0.1 * np.arange(E)[:, None]
    q0[:, :, 2] = 0.1 - 0.002 * (1 + np.arange(E))[:, None]
    order = [4, 0, 3, 1, 2]

    def uncut_and_state():
        with rb.BatchWorld(sc, E) as whole:
            whole.set_state(q0, v0)
            for _ in range(5):                      # stepped until contacts exist
                assert whole.step(1) == 0
                if whole.contacts(max_records=0).counts.min() > 0:
                    break
            return whole.contacts(max_records=R), whole.contacts(envs=order, max_records=R), whole.get_state()

    ref, ref_order, (q, v) = uncut_and_state()
    assert ref.counts.min() > 0 and ref.truncated == 0
    assert len({_words(ref.dist[e]).tobytes() for e in range(E)}) == E
    assert not differing(ref_order, {f: getattr(ref, f)[order] for f in FIELDS})
    monkeypatch.setenv("RBHIP_BATCH_SAMPLE_BYTES", str(2 * per))
    with rb.BatchWorld(sc, E) as b:
        b.set_state(q, v)
        cut = b.contacts(envs=order, max_records=R)
        assert not differing(cut, {f: getattr(ref_order, f) for f in FIELDS}) and cut.truncated == ref_order.truncated
        cut = b.contacts(max_records=R)
        assert not differing(cut, {f: getattr(ref, f) for f in FIELDS}) and cut.truncated == ref.truncated
    monkeypatch.setenv("RBHIP_BATCH_SAMPLE_BYTES", str(per - 1))
    with rb.BatchWorld(sc, E) as b:
        b.set_state(q, v)
        arrays = [np.full((E, M), 7, np.int32), np.full((E, M, R), 7, np.int32), np.full((E, M, R), 7, np.int32),
                  np.full((E, M, R), 7.0), np.full((E, M, R, 3), 7.0), np.full((E, M, R, 3), 7.0)]
        nt = C.c_int64()
        rc = b._L.rb_batch_contacts(b._h, None, E, R, *(rb._lib.ptr(a) for a in arrays), C.byref(nt))
        assert rc == EINVAL and b"do not fit the staging buffer" in b._L.rb_last_error()
        assert all((a == 7).all() for a in arrays)
        with pytest.raises(rb.RbError) as ei:
            b.contacts(max_records=R)
        assert ei.value.code == EINVAL
        assert np.array_equal(b.contacts(max_records=0).counts, ref.counts)      # (the counts alone fit)


# ------------------------------------------------------------ 8. many partners
def test_many_partners(rb, oracle):
    """24 spheres of r 0.1 within +-0.03 of one point (the cluster of
    test_gpu_batch.py::test_more_partners_than_a_world_allows): 23 partners
    per body, R = 32."""
    from rbhip import scenes
    sc = scenes.flat_spheres(6, 4)
    E, M = 2, sc.n
    rng = np.random.default_rng(12)
    q = np.zeros((E, M, 7))
    q[:, :, 0:3] = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.03, 0.03, (E, M, 3))
    q[:, :, 3] = 1.0
    v = np.broadcast_to(sc.qvel0, (E, M, 6)).copy()
    with rb.BatchWorld(sc, E) as b:
        b.set_state(q, v)
        for n in (0, 5):
            assert b.step(n) == 0
            gq, _ = b.get_state()
            con = b.contacts(max_records=32)
            ref, kinds = oracle_dense(oracle, [sc] * E, gq, 32)
            # (all 24 within 0.104 of each other at the start, touching below 0.2: still in a cluster 5 steps on)
            assert (ref["counts"] == 23).all() if n == 0 else ref["counts"].min() >= 12
            assert kinds[16] == ref["counts"].sum()
            assert not differing(con, ref) and con.truncated == 0


# ------------------------------------------------------------ 9. a failed environment
def test_failed_environment(rb, oracle):
    scs = column_scenes()
    q0 = np.stack([sc.qpos0 for sc in scs])
    v0 = np.stack([sc.qvel0 for sc in scs])
    q0[5, 2, 2] = np.nan
    others = [k for k in range(E_COL) if k != 5]
    with rb.BatchWorld.from_scenes(scs) as b:
        b.set_state(q0, v0)
        assert b.step(150) == 1
        code, done = b.status()
        assert code[5] == EDOM and done[5] == 0 and not code[others].any()
        q, _ = b.get_state()
        con = b.contacts(max_records=8)
    assert (con.counts[5] == -1).all() and (con.kind[5] == -1).all() and not con.partner[5].any()
    assert not _words(con.dist[5]).any() and not _words(con.pos[5]).any() and not _words(con.frame[5]).any()
    ref, kinds = oracle_dense(oracle, [scs[k] for k in others], q[others], 8)
    assert_box_floors(kinds, 10, 30)
    assert not differing(con, ref, got_rows=others)
    assert con.truncated == 0


# ------------------------------------------------------------ 10. the query changes nothing
def test_query_changes_nothing(rb):
    import torch
    scs = column_scenes()
    with rb.BatchWorld.from_scenes(scs) as a, rb.BatchWorld.from_scenes(scs) as b:
        for w in (a, b):
            assert w.step(100) == 0
        before = a.get_state()
        host = a.contacts(max_records=8)
        dev = a.contacts_device(max_records=8)
        assert a.sync() == 0
        assert host.counts.sum() > 0 and np.array_equal(dev.counts.cpu().numpy(), host.counts)
        after = a.get_state()
        assert all(np.array_equal(_words(x), _words(y)) for x, y in zip(before, after))
        for w in (a, b):
            assert w.step(300) == 0                      # 256 + 44: across a launch cut
        sa, sb = a.get_state(), b.get_state()
        assert all(np.array_equal(_words(x), _words(y)) for x, y in zip(sa, sb))
        (ca, da), (cb, db) = a.status(), b.status()
        assert np.array_equal(ca, cb) and np.array_equal(da, db) and (da == 400).all()
    assert torch is not None


# ------------------------------------------------------------ 11. device form
def test_device_form(rb, column):
    """contacts_device on a stream of the caller, enqueued right after
    step_async with no sync in between, float64 and float32 element types,
    new tensors and preallocated ones."""
    import torch
    scs = column["scs"]
    stream = torch.cuda.Stream()
    with rb.BatchWorld.from_scenes(scs) as b:
        b.use_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            pre = rb.BatchContacts(8, torch.full((E_COL, 4), 77, dtype=torch.int32, device="cuda"),
                                   *(torch.full((E_COL, 4, 8), 77, dtype=torch.int32, device="cuda") for _ in range(2)),
                                   torch.full((E_COL, 4, 8), 7.0, dtype=torch.float32, device="cuda"),
                                   *(torch.full((E_COL, 4, 8, 3), 7.0, dtype=torch.float32, device="cuda") for _ in range(2)),
                                   None)
            ptrs = [getattr(pre, f).data_ptr() for f in FIELDS]
            b.step_async(150)
            d64 = b.contacts_device(max_records=8)
            d32 = b.contacts_device(out=pre)
            cnt = b.contacts_device(max_records=0)
            nogeo = b.contacts_device(max_records=8, geometry=False, dtype="f32")
        assert b.sync() == 0
        host = b.contacts(max_records=8)
    d = column["at"][150]
    assert not differing(host, d["ref"])
    assert d64.truncated is None and d64.dist.dtype == torch.float64 and d64.pos.shape == (E_COL, 4, 8, 3)
    assert not differing(rb.BatchContacts(8, *(getattr(d64, f).cpu().numpy() for f in FIELDS), None), d["ref"])
    assert d32.counts is pre.counts and d32.frame is pre.frame and [getattr(pre, f).data_ptr() for f in FIELDS] == ptrs
    for f in FIELDS:
        got = getattr(d32, f).cpu().numpy()
        want = getattr(host, f)
        assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32) if f in FLOAT_FIELDS
                              else want.view(np.uint32)), f
    assert cnt.partner is None and np.array_equal(cnt.counts.cpu().numpy(), host.counts)
    assert nogeo.pos is None and nogeo.frame is None and nogeo.dist.dtype == torch.float32
    assert np.array_equal(nogeo.dist.cpu().numpy(), host.dist.astype(np.float32))
    assert np.array_equal(nogeo.kind.cpu().numpy(), host.kind)


# ------------------------------------------------------------ 12. an f32 batch
def test_f32_batch(rb, oracle):
    """The column sweep in f32 against the oracle's fp32 restatement.  A CPU
    run of that oracle lists 42 / 60 / 54 / 38 / 30 / 34 records of kinds 17 /
    32..35 / 40 and 57 corners at step 150."""
    scs = column_scenes()
    with rb.BatchWorld.from_scenes(scs, dtype="f32") as b:
        assert b.step(150) == 0
        q, _ = b.get_state()
        con = b.contacts(max_records=8)
    assert np.array_equal(q, q.astype(np.float32).astype(np.float64))
    ref, kinds = oracle_dense(oracle, scs, q, 8, dtype="f32")
    assert_box_floors(kinds, 10, 30)
    assert ref["counts"].max() == 8
    assert not differing(con, ref, exact_words=False)


# ------------------------------------------------------------ 13. refusals on a live batch
def test_refusals_on_a_live_batch(rb):
    import ctypes as C
    from rbhip import _lib, scenes
    sc = scenes.ball_collision()
    with rb.BatchWorld(sc, 3, law="balls") as b:
        for call in (b.contacts, lambda: b.contacts_device(max_records=2)):
            with pytest.raises(rb.RbError) as ei:
                call()
            assert ei.value.code == EUNSUPPORTED
        assert b.step(20) == 0
        b.set_contact_law("mujoco")
        assert b.contacts().counts.shape == (3, 2)
    sc = scenes.multi_sphere4()
    with rb.BatchWorld(sc, 5) as b:
        L, h = b._L, b._h
        cnt, rec, dis = np.full((5, 4), 99, np.int32), np.full((5, 4, 2), 99, np.int32), np.full((5, 4, 2), 9.0)
        c, r, d = _lib.ptr(cnt), _lib.ptr(rec), _lib.ptr(dis)
        ids = lambda *a: _lib.ptr(np.array(a, np.int64))     # noqa: E731
        refused = [(None, 5, -1, c, r, r, d, None, None, None),       # max_records < 0
                   (None, 5, 0, c, r, r, d, None, None, None),        # max_records 0 with record arrays
                   (None, 5, 2, c, None, None, None, None, None, None),
                   (None, 5, 2, c, r, None, d, None, None, None),     # not all together
                   (None, 5, 2, None, r, r, d, None, None, None),     # counts is required
                   (ids(0), -1, 2, c, r, r, d, None, None, None),     # n < 0
                   (None, 4, 2, c, r, r, d, None, None, None),        # all environments: n = n_envs
                   (ids(0, 5), 2, 2, c, r, r, d, None, None, None),   # out of range
                   (ids(1, -1), 2, 2, c, r, r, d, None, None, None),
                   (ids(3, 1, 3), 3, 2, c, r, r, d, None, None, None)]    # listed twice
        for args in refused:
            assert L.rb_batch_contacts(h, *args) == EINVAL, args
        assert (cnt == 99).all() and (rec == 99).all() and (dis == 9.0).all()
        # the device form: a host pointer, an unknown element type
        assert L.rb_batch_contacts_dev(h, 2, c, r, r, d, None, None, 0) == EINVAL
        assert b"not device memory" in L.rb_last_error()
        assert L.rb_batch_contacts_dev(h, 2, c, r, r, d, None, None, 7) == EINVAL
        with pytest.raises(TypeError, match="counts"):
            b.contacts_device(out=dict(counts=cnt, partner=None))
        with pytest.raises(TypeError, match="partner"):
            b.contacts_device(out=dict(counts=cnt, partner=rec, kind=rec, dist=dis))
        assert b.step(10) == 0 and C is not None
        assert b.contacts(max_records=2).counts.shape == (5, 4)
