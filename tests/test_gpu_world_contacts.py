"""The contact query of a World (World.query_contacts, query_contacts_device;
rb_query_contacts, rb_query_contacts_dev): the contact list of the current
state, without a step, with pos and frame.

1. against the oracle and the long-double all-pairs reference of
   tests/contact_geometry.py, word for word, for states set with set_state;
2. equal to the batch's query of the same state;
3. equal to the list a step records, through every step form;
4. purity: a world that is queried between its runs steps to the same bits
   and the same stats as one that is not;
5. ranges, truncation, fill, geometry switches;
6. the device form: float32 outputs, stream order, out=;
7. bodies without a list (-2): more than 32 partners, a NaN position;
8. refusals.
"""
import ctypes as C

import numpy as np
import pytest

import contact_geometry as cg
import test_gpu_contact_geometry as tcg

pytestmark = pytest.mark.gpu

EINVAL, EOVERFLOW, EUNSUPPORTED, EDOM = -22, -75, -95, -33
FIELDS = ("counts", "partner", "kind", "dist", "pos", "frame")
_same, _case, _setenv = tcg._same, tcg._case, tcg._setenv


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _equal(a, b):
    """Two queries (or tuples of arrays), word for word in every field."""
    ta = tuple(getattr(a, f) for f in FIELDS) if hasattr(a, "counts") else tuple(a)
    tb = tuple(getattr(b, f) for f in FIELDS) if hasattr(b, "counts") else tuple(b)
    bad = []
    for f, x, y in zip(FIELDS, ta, tb):
        if (x is None) != (y is None):
            bad.append(f)
        elif x is not None and (np.shape(x) != np.shape(y) or not np.array_equal(_words(x), _words(y))):
            bad.append(f)
    return bad


def _fill_ok(con):
    """Every slot at or past a body's count holds kind -1 and zeros."""
    cnt = np.asarray(con.counts).reshape(-1)
    R = con.max_records
    unused = ~(np.arange(R)[None, :] < np.clip(cnt, 0, R)[:, None])
    n = cnt.size
    ok = (np.asarray(con.kind).reshape(n, R)[unused] == -1).all() and not np.asarray(con.partner).reshape(n, R)[unused].any()
    ok = ok and not _words(np.asarray(con.dist).reshape(n, R)[unused]).any()
    for a in (con.pos, con.frame):
        if a is not None:
            ok = ok and not _words(np.asarray(a).reshape(n, R, 3)[unused]).any()
    used = ~unused
    return bool(ok) and bool((np.asarray(con.kind).reshape(n, R)[used] >= 0).all())


# ------------------------------------------------------------ 1. oracle and reference
WORLD_PLANE_N = tcg.WORLD_PLANE_N
MIXED_M = 1043                                   # one world of the mixed family's bodies, no multiple of 64
PLANES = ["plane_random", "plane_diagonal", "plane_deep", "plane_spheres"]
REFERENCE = [(f, "f64") for f in list(cg.CELL_FAMILIES) + PLANES + ["pairs_grazing", "pairs_coincident", "mixed"]] + \
            [(f, "f32") for f in cg.CELL_FAMILIES]


def _problem(family, dtype):
    if family in PLANES:
        return cg.make(family, n=WORLD_PLANE_N, M=WORLD_PLANE_N, dtype=dtype)
    if family == "mixed":
        return cg.mixed(1, seed=305, M=MIXED_M)
    return cg.make(family, dtype=dtype)


@pytest.mark.parametrize("family,dtype", REFERENCE, ids=[f"{f}-{d}" for f, d in REFERENCE])
def test_query_against_oracle_and_reference(rb, oracle, family, dtype):
    key = ("world", family, dtype) if family != "mixed" else ("world-query", family, dtype)
    pb, ref, want = _case(oracle, key, lambda: _problem(family, dtype), dtype)
    assert pb.G == 1 and pb.N % 64 != 0 and want[0].sum() > 0
    # the query searches with 32 partners whatever the world was made with
    # (radius_mix: 24 touching partners per big sphere, a world of max_partners 16)
    with rb.World(pb.scene(0), dtype=dtype, max_partners=16) as w:
        w.set_state(pb.qpos, np.zeros((pb.N, 6)))
        con = w.query_contacts()
        assert con.truncated == 0 and con.counts.shape == (1, pb.N) and _fill_ok(con)
        got = cg.dense_lists(con)
        assert not _equal(got, con.to_csr())
    if family == "radius_mix":
        assert want[0].max() >= 24
    cg.assert_properties(got, pb, dtype, ref)
    assert not _same(got, want, dtype)


# ------------------------------------------------------------ 2. equals the batch
def _batch_scene(name):
    from rbhip import scenes
    return {"column": lambda: scenes.box_pile(1, 1, 3), "mixed14": lambda: scenes.box_pile(2, 2, 3),
            "wide70": lambda: scenes.box_pile(4, 4, 4), "spheres64": lambda: scenes.flat_spheres(8, 8, spacing=0.19)}[name]()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["column", "mixed14", "wide70", "spheres64"])
def test_query_equals_the_batch(rb, name, dtype):
    sc = _batch_scene(name)
    assert sc.n == {"column": 4, "mixed14": 14, "wide70": 70, "spheres64": 64}[name]
    with rb.World(sc, dtype=dtype, max_partners=32) as w:
        w.step(50)
        q, v = w.get_state()
        con = w.query_contacts(max_records=32)
    with rb.BatchWorld.from_scenes([sc], dtype=dtype) as b:
        b.set_state(q[None], v[None])
        ref = b.contacts(max_records=32)
    assert con.counts.sum() > 0 and con.truncated == ref.truncated == 0
    assert not _equal(con, ref)


# ------------------------------------------------------------ 3. equals the recorded list
@pytest.mark.parametrize("form", list(tcg.FORMS))
@pytest.mark.parametrize("family", ["cells_negative", "mixed"])
def test_query_equals_the_recorded_list(rb, oracle, monkeypatch, family, form):
    code, env = tcg.FORMS[form]
    _setenv(monkeypatch, env)
    key = ("world", family, "f64") if family != "mixed" else ("world-query", family, "f64")
    pb, _, _ = _case(oracle, key, lambda: _problem(family, "f64"), "f64")
    with rb.World(pb.scene(0), max_partners=pb.max_partners) as w:
        w.set_state(pb.qpos, np.zeros((pb.N, 6)))
        con = w.query_contacts()
        w.record_contacts(True)
        w.step(1)
        rec = w.contacts()
        st = w.stats()
    assert st["hashed_form"] == code, st
    assert con.truncated == 0 and rec[0].sum() > 0
    assert not _same(rec, con.to_csr()[:4], "f64")


# ------------------------------------------------------------ 4. purity
PURE_FORMS = {"coop_help": tcg.FORMS["coop_help"], "wide": tcg.FORMS["wide"], "one": tcg.FORMS["one"]}


def _runs(rng, total=60, lo=1, hi=7):
    out = []
    while sum(out) < total:
        out.append(int(min(rng.integers(lo, hi + 1), total - sum(out))))
    if out[-1] < lo:                             # (the tile case: no run shorter than lo)
        out[-2] += out.pop()
    return out


def _interleave(rb, torch, oracle, sc, q0, v0, runs, seed, max_partners, check=None):
    """Worlds A and B step the same runs; A is queried between them.  After
    every run: the same state in uint64, the same stats key for key."""
    rng = np.random.default_rng(seed)
    n = sc.n
    with rb.World(sc, max_partners=max_partners) as A, rb.World(sc, max_partners=max_partners) as B:
        for w in (A, B):
            w.set_state(q0, v0)
        held, asked = [], 0
        for r, k in enumerate(runs):
            for _ in range(int(rng.integers(1, 4))):
                R = int(rng.choice([0, 1, 8]))
                first = int(rng.integers(0, n - 1))
                count = int(rng.integers(1, n - first + 1))
                if asked % 2 == 0:
                    con = A.query_contacts(first, count, max_records=R, strict=False)
                    assert con.counts.shape == (1, count) and con.counts.min() >= 0
                else:                            # (enqueued only; the tensors live until the stream has run)
                    held.append(A.query_contacts_device(first, count, max_records=R))
                asked += 1
            A.step(k)
            B.step(k)
            held.clear()                         # (step() waited for the stream)
            qa, va = A.get_state()
            qb, vb = B.get_state()
            assert np.array_equal(_words(qa), _words(qb)) and np.array_equal(_words(va), _words(vb)), (r, k)
            sa, sb = A.stats(), B.stats()
            assert sa == sb, (r, {key: (sa[key], sb[key]) for key in sa if sa[key] != sb.get(key)})
            if check:
                check(A, qa)
        assert asked >= len(runs)
        return A.stats()


@pytest.mark.parametrize("form", list(PURE_FORMS))
@pytest.mark.parametrize("name", ["spheres1100", "pile14"])
def test_queries_change_nothing_a_step_can_see(rb, torch, oracle, monkeypatch, name, form):
    from rbhip import scenes
    code, env = PURE_FORMS[form]
    _setenv(monkeypatch, env)
    sc = scenes.flat_spheres(44, 25, seed=3, spacing=0.21) if name == "spheres1100" else scenes.box_pile(2, 2, 3)
    assert sc.n == (1100 if name == "spheres1100" else 14) and np.any(sc.gravity != 0)
    runs = _runs(np.random.default_rng(11))
    assert sum(runs) == 60 and min(runs) >= 1 and max(runs) <= 7
    st = _interleave(rb, torch, oracle, sc, sc.qpos0, sc.qvel0, runs, 12, 32)
    assert st["hashed_form"] == code, st
    if form == "wide" and name == "spheres1100":
        assert st["table_epoch"] > 1 and st["append_steps"] > 0, st      # epochs on (the default)


def test_queries_change_nothing_in_the_tile_form(rb, torch, oracle, monkeypatch):
    _setenv(monkeypatch, {"RBHIP_TILE": "1"})
    pb, _, _ = _case(oracle, ("world", "cells_half", "f64"), lambda: cg.make("cells_half"), "f64")
    sc = pb.scene(0)
    osc = oracle.OracleScene(sc, max_partners=pb.max_partners)

    def check(w, q):                             # the query after a tile run: the oracle's lists of get_state()
        got = cg.dense_lists(w.query_contacts())
        assert not _same(got, oracle.contacts(osc, q), "f64")

    runs = _runs(np.random.default_rng(13), lo=2)
    assert sum(runs) == 60 and min(runs) >= 2
    st = _interleave(rb, torch, oracle, sc, pb.qpos, np.zeros((pb.N, 6)), runs, 14, pb.max_partners, check)
    assert st["form"] == 5 and st["tile_rollbacks"] == 0 and st["tile_steps"] == 60, st


def test_query_follows_a_refit_and_a_grown_table(rb, oracle, monkeypatch):
    """The query's table is made for the world's grid as it stands: a guarded
    chunk with two injected bucket overflows refits the layout and doubles the
    table between two queries, and both equal the oracle's lists."""
    from rbhip import scenes
    _setenv(monkeypatch, tcg.FORMS["wide"][1])
    monkeypatch.setenv("RBHIP_DIAG_OVERFLOW", "2")
    sc = scenes.flat_spheres(44, 25, seed=3, spacing=0.21)
    osc = oracle.OracleScene(sc, max_partners=32)
    with rb.World(sc, max_partners=32) as w:
        w.step(40)
        st0 = w.stats()
        q, _ = w.get_state()
        before = w.query_contacts(max_records=16)
        assert before.counts.sum() > 0 and not _same(cg.dense_lists(before), oracle.contacts(osc, q), "f64")
        w.step(70)                               # guarded: rolled back twice, refitted, the table doubled
        st = w.stats()
        assert st["refits"] == 2 and st["table_grows"] == 1 and st["buckets"] == 2 * st0["buckets"], (st0, st)
        q, _ = w.get_state()
        after = w.query_contacts(max_records=16)
        assert after.counts.sum() > 0 and not _same(cg.dense_lists(after), oracle.contacts(osc, q), "f64")


# ------------------------------------------------------------ 5. ranges, truncation, fill
@pytest.fixture(scope="module")
def negative(rb, oracle):
    """cells_negative in a world, and its full query."""
    pb, _, want = _case(oracle, ("world", "cells_negative", "f64"), lambda: cg.make("cells_negative"), "f64")
    w = rb.World(pb.scene(0), max_partners=pb.max_partners)
    w.set_state(pb.qpos, np.zeros((pb.N, 6)))
    full = w.query_contacts()
    assert not _same(cg.dense_lists(full), want, "f64")
    yield w, pb, full
    w.close()


def test_ranges_truncation_and_fill(rb, negative):
    w, pb, full = negative
    N, R = pb.N, full.max_records
    assert R == 4 * 3 + 32 and full.counts.max() > 1 and _fill_ok(full)
    part = w.query_contacts(first=37, count=N - 100)
    assert part.first == 37 and part.max_records == R
    want = rb.WorldContacts(R, *(getattr(full, f)[:, 37:N - 63] for f in FIELDS), None)
    assert not _equal(part, want) and part.truncated == 0
    one = w.query_contacts(max_records=1)
    assert not _equal((one.counts,), (full.counts,)) and one.truncated == int((full.counts > 1).sum()) > 0
    first = rb.WorldContacts(1, full.counts, *(getattr(full, f)[:, :, :1] for f in FIELDS[1:]), None)
    assert not _equal(one, first) and _fill_ok(one)
    none = w.query_contacts(max_records=0)
    assert none.partner is None and none.dist is None and none.pos is None and none.max_records == 0
    assert not _equal((none.counts,), (full.counts,)) and none.truncated == int((full.counts > 0).sum())
    flat = w.query_contacts(geometry=False)
    assert flat.pos is None and flat.frame is None
    assert not _equal(tuple(getattr(flat, f) for f in FIELDS[:4]), tuple(getattr(full, f) for f in FIELDS[:4]))
    # pos alone and frame alone, through the raw binding
    for which in ("pos", "frame"):
        cnt = np.zeros(N, np.int32)
        par, kin, dis = np.zeros((N, R), np.int32), np.zeros((N, R), np.int32), np.zeros((N, R))
        geo = np.full((N, R, 3), 7.5)
        p = rb._lib.ptr
        rc = w._L.rb_query_contacts(w._h, 0, N, R, p(cnt), p(par), p(kin), p(dis), p(geo) if which == "pos" else None,
                                    p(geo) if which == "frame" else None, None)
        assert rc == 0, w._L.rb_last_error()
        got = (cnt[None], par[None], kin[None], dis[None], geo[None])
        ref = tuple(getattr(full, f) for f in FIELDS[:4]) + (getattr(full, which),)
        assert not _equal(got, ref), which


def test_host_form_in_sub_ranges_under_a_small_staging_bound(rb, negative, monkeypatch):
    """A staging bound of 64 KiB cuts the request into launches over sub-ranges;
    a bound below one body's slots is RB_EINVAL."""
    _, pb, full = negative
    monkeypatch.setenv("RBHIP_CONTACT_STAGE_BYTES", str(64 << 10))
    with rb.World(pb.scene(0), max_partners=pb.max_partners) as w:
        w.set_state(pb.qpos, np.zeros((pb.N, 6)))
        per = 8 * 44 * 7 + 4 * (1 + 2 * 44)
        assert (64 << 10) // per < pb.N // 20                          # more than 20 launches
        assert not _equal(w.query_contacts(max_records=44), full)
    monkeypatch.setenv("RBHIP_CONTACT_STAGE_BYTES", "256")
    with rb.World(pb.scene(0), max_partners=pb.max_partners) as w:
        with pytest.raises(rb.RbError, match="EINVAL.*staging"):
            w.query_contacts(max_records=44)
        small = w.query_contacts()                                      # (None: capped by the bound)
        assert 0 < small.max_records < 44


# ------------------------------------------------------------ 6. the device form
def _host_con(rb, dev):
    """A device query's arrays on the host, reals widened to double."""
    ints = [getattr(dev, f).cpu().numpy() for f in FIELDS[:3]]
    reals = [None if getattr(dev, f) is None else getattr(dev, f).cpu().numpy().astype(np.float64) for f in FIELDS[3:]]
    return rb.WorldContacts(dev.max_records, *ints, *reals, None)


# float32 outputs round pos to the float32 grid at the body's place: the
# properties at the fp32 bounds hold within the few metres of the origin those
# bounds were measured for, which the clouds are and the 2 km row
# of the mixed world is not; the oracle's values rounded are asked of all three.
@pytest.mark.parametrize("family,near_origin", [("cells_negative", True), ("radius_mix", True), ("mixed", False)])
def test_device_form_float32_outputs(rb, torch, oracle, family, near_origin):
    """An fp64 world's lists written as float32: the fp64 problem's properties
    at the fp32 bounds, and the oracle's values rounded."""
    key = ("world", family, "f64") if family != "mixed" else ("world-query", family, "f64")
    pb, ref, want = _case(oracle, key, lambda: _problem(family, "f64"), "f64")
    assert (np.abs(pb.qpos[:, :3]).max() < 8.0) == near_origin
    with rb.World(pb.scene(0), max_partners=pb.max_partners) as w:
        w.set_state(pb.qpos, np.zeros((pb.N, 6)))
        dev = w.query_contacts_device(max_records=32, dtype="f32")
        w.sync()
        assert dev.truncated is None and dev.dist.dtype == torch.float32 and dev.frame.dtype == torch.float32
        host = _host_con(rb, dev)
    got = cg.dense_lists(host)
    if near_origin:
        cg.assert_properties(got, pb, "f32", ref)
    rounded = want[:3] + tuple(a.astype(np.float32).astype(np.float64) for a in want[3:])
    assert not _same(got, rounded, "f32")


def test_device_form_stream_order_and_out(rb, torch, oracle):
    from rbhip import scenes
    sc = scenes.flat_spheres(20, 15, seed=5, spacing=0.19)
    osc = oracle.OracleScene(sc, max_partners=32)
    rng = np.random.default_rng(6)
    q0 = sc.qpos0.copy()
    q0[:, 2] = rng.uniform(0.05, 0.3, sc.n)                 # low: ground and neighbour contacts from the start
    v0 = sc.qvel0.copy()
    q3, _ = oracle.step(osc, q0, v0, 3)
    want0, want3 = oracle.contacts(osc, q0), oracle.contacts(osc, q3)
    assert want0[0].sum() > sc.n // 2 and want3[0].sum() > 0 and want0[0].max() <= 16
    with rb.World(sc, max_partners=32) as w:
        w.set_stream(torch.cuda.current_stream().cuda_stream)
        dq, dv = torch.from_numpy(q0).to("cuda:0"), torch.from_numpy(v0).to("cuda:0")
        # nothing waits between these five
        w.set_state_device(dq, dv, refit=False)
        a = w.query_contacts_device(max_records=16)
        w.step_async(3)
        b = w.query_contacts_device(max_records=16)
        w.sync()
        assert not _same(cg.dense_lists(_host_con(rb, a)), want0, "f64")
        assert not _same(cg.dense_lists(_host_con(rb, b)), want3, "f64")
        # out=: the given tensors are written and returned
        ptrs = {f: getattr(a, f).data_ptr() for f in FIELDS}
        for f in FIELDS:
            getattr(a, f).fill_(-3)
        again = w.query_contacts_device(out=a)
        w.sync()
        assert again.max_records == 16 and all(getattr(again, f).data_ptr() == ptrs[f] for f in FIELDS)
        assert not _equal(_host_con(rb, again), _host_con(rb, b))
        with pytest.raises(ValueError, match="max_records"):
            w.query_contacts_device(max_records=8, out=a)
        counts_only = w.query_contacts_device(out={"counts": a.counts})
        w.sync()
        assert counts_only.partner is None and np.array_equal(counts_only.counts.cpu().numpy(), b.counts.cpu().numpy())


# ------------------------------------------------------------ 7. no list
def _ring_scene(n_small=40):
    """One r = 1.0 sphere ringed by n_small touching r = 0.05 ones (0.002 into
    it, 0.16 apart along the ring: no two of them touch)."""
    a = 2 * np.pi * np.arange(n_small) / n_small
    c = np.concatenate([[[0.0, 0.0, 0.0]], 1.048 * np.stack([np.cos(a), np.sin(a), 0 * a], 1)]) + [0.3, -0.2, 2.0]
    r = np.array([1.0] + [0.05] * n_small)
    return cg._cloud("ring", c, r=r, max_partners=32)


def _small_lists(oracle, pb):
    """The oracle's list of every small sphere: its pair with body 0 as a scene
    of two bodies (no two small spheres touch; the partner keeps id 0)."""
    parts = []
    for k in range(1, pb.N):
        sub = cg.Problem("pair", 2, pb.kind[[0, k]], pb.size[[0, k]], pb.qpos[[0, k]], pb.planes)
        cnt, *rest = cg.oracle_lists(oracle, sub)
        assert cnt.tolist() == [1, 1]
        parts.append(tuple(x[1:2] for x in (cnt,) + tuple(rest)))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(6))


def test_more_than_32_partners_is_a_body_without_a_list(rb, torch, oracle):
    pb = _ring_scene()
    assert pb.N == 41
    want = _small_lists(oracle, pb)
    zeros = np.zeros((pb.N, 6))
    with rb.World(pb.scene(0), max_partners=32) as w, rb.World(pb.scene(0), max_partners=32) as twin:
        w.set_state(pb.qpos, zeros)
        twin.set_state(pb.qpos, zeros)
        with pytest.raises(rb.RbError, match=r"EOVERFLOW.*body 0 ") as exc:
            w.query_contacts()
        assert exc.value.code == EOVERFLOW
        con = w.query_contacts(strict=False)
        assert con.counts[0, 0] == -2 and (con.counts[0, 1:] == 1).all() and _fill_ok(con)
        assert con.kind[0, 0].tolist() == [-1] * con.max_records and con.truncated == 0
        small = rb.WorldContacts(con.max_records, *(getattr(con, f)[:, 1:] for f in FIELDS), 0)
        assert not _same(cg.dense_lists(small), want, "f64")
        dev = w.query_contacts_device(max_records=con.max_records)
        w.sync()
        assert not _equal(_host_con(rb, dev), con)
        # The world's error word was not touched.  (The step finds the same 40
        # partners and overflows its own list of 32: it is refused in the
        # world that was queried exactly as in its twin that never was, and
        # leaves no error behind in either.)
        outcomes = []
        for x in (w, twin):
            try:
                x.step(1)
                outcomes.append(("ok", 0))
            except rb.RbError as e:
                outcomes.append(("error", e.code))
        assert outcomes[0] == outcomes[1], outcomes
    # 30 touching partners: every body has a list, and a following step succeeds
    pb = _ring_scene(30)
    with rb.World(pb.scene(0), max_partners=32) as w:
        w.set_state(pb.qpos, np.zeros((pb.N, 6)))
        con = w.query_contacts()
        assert con.counts[0].tolist() == [30] + [1] * 30
        w.step(1)


def test_a_nan_position_is_a_body_without_a_list(rb, torch):
    from rbhip import scenes
    sc = scenes.flat_spheres(8, 8)
    with rb.World(sc) as w:
        clean = w.query_contacts(max_records=4)
        q = sc.qpos0.copy()
        q[5, 0] = np.nan
        w.set_state(q, sc.qvel0)
        with pytest.raises(rb.RbError, match=r"EDOM.*body 5 ") as exc:
            w.query_contacts(max_records=4)
        assert exc.value.code == EDOM
        con = w.query_contacts(max_records=4, strict=False)
        assert con.counts[0, 5] == -2 and (np.delete(con.counts[0], 5) >= 0).all() and _fill_ok(con)
        assert not (clean.partner == 5).any()                # (no list of the clean state names body 5)
        keep = np.arange(sc.n) != 5
        assert not _equal(tuple(getattr(con, f)[:, keep] for f in FIELDS), tuple(getattr(clean, f)[:, keep] for f in FIELDS))
        dev = w.query_contacts_device(max_records=4)
        w.sync()
        assert not _equal(_host_con(rb, dev), con)
        # a range that leaves the body out has nothing to report
        assert w.query_contacts(first=6, max_records=4).counts.min() >= 0


# ------------------------------------------------------------ 8. refusals
def test_refusals(rb, torch):
    from rbhip import scenes
    sc = scenes.flat_spheres(8, 8, spacing=0.19)
    N, R = sc.n, 4
    cnt, par, kin = np.zeros(N, np.int32), np.zeros((N, R), np.int32), np.zeros((N, R), np.int32)
    dis, geo = np.zeros((N, R)), np.zeros((N, R, 3))
    p = rb._lib.ptr
    d = {k: torch.zeros(s, dtype=t, device="cuda:0") for k, s, t in
         (("cnt", (N,), torch.int32), ("par", (N, R), torch.int32), ("kin", (N, R), torch.int32),
          ("dis", (N, R), torch.float64), ("geo", (N, R, 3), torch.float64))}
    dp = {k: C.c_void_p(v.data_ptr()) for k, v in d.items()}
    with rb.World(sc) as w:
        w.step(30)
        L, h = w._L, w._h
        base = w.query_contacts(max_records=R)
        q0, v0 = w.get_state()
        st0 = w.stats()

        def host(first=0, count=N, r=R, c=p(cnt), a=p(par), k=p(kin), x=p(dis), g=p(geo), f=None, hh=h):
            return L.rb_query_contacts(hh, first, count, r, c, a, k, x, g, f, None)

        def dev(first=0, count=N, r=R, c=dp["cnt"], a=dp["par"], k=dp["kin"], x=dp["dis"], g=dp["geo"], f=None, io=0, hh=h):
            return L.rb_query_contacts_dev(hh, first, count, r, c, a, k, x, g, f, io)

        refused = [
            ("null world", lambda f: f(hh=None)), ("counts", lambda f: f(c=None)), ("max_records < 0", lambda f: f(r=-1)),
            ("max_records 0", lambda f: f(r=0)), ("max_records 0", lambda f: f(r=0, a=None, k=None, x=None)),
            ("max_records 4", lambda f: f(a=None, k=None, x=None, g=None)), ("only all together", lambda f: f(k=None)),
            ("outside", lambda f: f(first=-1)), ("outside", lambda f: f(count=-1)), ("outside", lambda f: f(first=1)),
            ("outside", lambda f: f(first=N + 1, count=0)),
        ]
        for form in (host, dev):
            for text, call in refused:
                assert call(form) == EINVAL, (form.__name__, text)
                assert text.encode() in L.rb_last_error(), (form.__name__, text, L.rb_last_error())
                assert not _equal(w.query_contacts(max_records=R), base), (form.__name__, text)
            assert form(first=N, count=0) == 0 and form(first=3, count=0) == 0
        assert dev(io=7) == EINVAL and b"io_dtype" in L.rb_last_error()
        # a host pointer given to the device form
        for name in ("c", "a", "x", "g"):
            hostp = {"c": p(cnt), "a": p(par), "x": p(dis), "g": p(geo)}[name]
            assert dev(**{name: hostp}) == EINVAL and b"not device memory" in L.rb_last_error(), name
        with pytest.raises(TypeError, match="counts"):
            w.query_contacts_device(out={"counts": cnt})
        w.sync()
        assert not any(t.any().item() for t in d.values())    # nothing was enqueued
        assert not _equal(w.query_contacts(max_records=R), base)
        assert all(np.array_equal(_words(a), _words(b)) for a, b in zip(w.get_state(), (q0, v0)))
        assert w.stats() == st0
    with rb.World(sc, rank=0, world_size=2) as w:
        assert w._L.rb_query_contacts(w._h, 0, 1, 0, p(cnt), None, None, None, None, None, None) == EUNSUPPORTED
        assert b"world_size" in w._L.rb_last_error()
        assert w._L.rb_query_contacts_dev(w._h, 0, 1, 0, dp["cnt"], None, None, None, None, None, 0) == EUNSUPPORTED
        with pytest.raises(rb.RbError, match="EUNSUPPORTED"):
            w.query_contacts()
    with rb.World(scenes.ball_collision(), law="balls") as w:
        with pytest.raises(rb.RbError, match="EUNSUPPORTED.*two-ball"):
            w.query_contacts()
        with pytest.raises(rb.RbError, match="EUNSUPPORTED"):
            w.query_contacts_device(max_records=0)
