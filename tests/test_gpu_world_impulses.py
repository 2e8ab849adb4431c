"""The impulse query of a World (World.query_impulses, query_impulses_device;
rb_query_impulses, rb_query_impulses_dev; kernels in rb_world_impulses.hip).

1. Against the CPU model (tests/impulse_model.py, itself held to the oracle's
   step by tests/test_impulse_model.py): every word of counts, partner, kind,
   dist, jn, jt, vel and net, f64 and f32, at states the world's own steps reach.
2. Against the step, no model: vel equals the qvel of the next step(1) in the
   hashed forms and the tile form, with applied forces, with the parameters of
   the call, under the raw normal convention.
3. Against the contact query: the four record fields word for word; every
   unused slot defined.
4. Ranges and truncation; the host form in sub-range launches.
5. Purity: a world queried between its runs steps to the same bits and stats.
6. Bodies without a list.  7. The device form.  8. Refusals.
"""
import ctypes as C
import warnings

import numpy as np
import pytest

import contact_geometry as cg
import impulse_model as IM
import test_gpu_contact_geometry as tcg
from test_gpu_contact_geometry import FORMS

pytestmark = pytest.mark.gpu

EINVAL, EOVERFLOW, EUNSUPPORTED, EDOM = -22, -75, -95, -33
RECORDS = ("counts", "partner", "kind", "dist")
FIELDS = ("counts", "partner", "kind", "dist", "jn", "jt", "vel", "net")
_setenv, _case = tcg._setenv, tcg._case
HASHED = {k: FORMS[k] for k in ("one", "coop_help", "wide")}


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _w(a):
    """The words of an array (reals as unsigned integers: the sign of zeros counts)."""
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_w(a), _w(b))


def differing(imp, ref, fields=FIELDS):
    """The fields of imp (a WorldImpulses / WorldContacts, or a mapping) that differ from ref's in any word."""
    get = lambda o, f: o[f] if isinstance(o, dict) else getattr(o, f)    # noqa: E731
    return [f for f in fields if not _same(get(imp, f), get(ref, f))]


def rows(imp, lo, hi):
    """The bodies [lo, hi) of a query, as a mapping."""
    return {f: None if getattr(imp, f) is None else getattr(imp, f)[:, lo:hi] for f in FIELDS}


def model_dense(sc, q, v, R, dtype="f64", **params):
    """The model of scene sc at (q, v) in the query's dense layout for one row, and the model itself."""
    m = IM.impulses(sc, q, v, dtype=dtype, max_partners=32, **params)
    counts, partner, kind, dist, jn, jt = IM.dense(m, R)
    return {f: a[None] for f, a in zip(FIELDS, (counts, partner, kind, dist, jn, jt, m.vel, m.net))}, m


def _fill_ok(imp):
    """Every slot at or past a body's count holds kind -1 and zero words, in jn and jt too."""
    cnt = np.asarray(imp.counts).reshape(-1)
    R, n = imp.max_records, cnt.size
    unused = ~(np.arange(R)[None, :] < np.clip(cnt, 0, R)[:, None])
    ok = (imp.kind.reshape(n, R)[unused] == -1).all() and not imp.partner.reshape(n, R)[unused].any()
    for a in (imp.dist, imp.jn):
        ok = ok and not _w(a.reshape(n, R)[unused]).any()
    ok = ok and not _w(imp.jt.reshape(n, R, 3)[unused]).any()
    return bool(ok) and bool((imp.kind.reshape(n, R)[~unused] >= 0).all())


def _scene(name):
    from rbhip import scenes
    return {"pile14": lambda: scenes.box_pile(2, 2, 3), "pile70": lambda: scenes.box_pile(4, 4, 4),
            "flat144": lambda: scenes.flat_spheres(12, 12, spacing=0.19), "mixed36": lambda: scenes.mixed_spheres(6, 6),
            "flat1100": lambda: scenes.flat_spheres(44, 25, seed=3, spacing=0.21)}[name]()


# ------------------------------------------------------------ 1. against the model
# Checked on the CPU with the oracle's steps, f64 and f32: every state has
# applied contacts; the piles and the flats have separating ones (16 of 31
# records at pile14 step 0, 38 of 147 at flat1100 step 60); mixed36, whose scene
# threshold is 1e-4, has threshold-skipped ones at step 150 (4 in f64, 1 in f32).
STATES = {"pile14": (0, 40, 120), "pile70": (0, 40), "flat144": (0, 30, 90), "mixed36": (60, 150), "flat1100": (60,)}
SEPARATING = ("pile14", "pile70", "flat144", "flat1100")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", list(STATES))
def test_every_word_equals_the_model(rb, oracle, name, dtype):
    sc = _scene(name)
    assert sc.n == int(name.lstrip("pileflatmxd"))
    separating = skipped = 0
    with rb.World(sc, dtype=dtype, max_partners=32) as w:
        done = 0
        for t in STATES[name]:
            w.step(t - done)
            done = t
            q, v = w.get_state()
            imp = w.query_impulses()
            R = imp.max_records
            assert R == 4 * len(sc.planes) + (4 if np.any(sc.kind != 0) else 1) * 32
            ref, m = model_dense(sc, q, v, R, dtype=dtype)
            print(f"{name} {dtype} step {t}: {int(m.counts.sum())} records, applied {m.applied}, "
                  f"separating {m.separating}, skipped {m.skipped}")
            assert m.applied > 0 and (ref["jn"] != 0).any(), t              # a state with no contact proves nothing
            assert not differing(imp, ref), t
            assert imp.truncated == 0 and imp.first == 0 and _fill_ok(imp)
            assert imp.counts.shape == (1, sc.n) and imp.jt.shape == (1, sc.n, R, 3) and imp.net.shape == (1, sc.n, 6)
            separating += m.separating
            skipped += m.skipped
    if name in SEPARATING:
        assert separating > 0
    if name == "mixed36":
        assert sc.threshold == 1e-4 and skipped > 0


# ------------------------------------------------------------ 2. against the step
def _vel_is_next_qvel(w, pre, queries=4, every=5, **params):
    """Query, step(1), compare, `queries` times `every` steps apart; returns the number of nonzero jn."""
    w.step(pre, **params)
    nonzero = 0
    for k in range(queries):
        imp = w.query_impulses(**params)
        w.step(1, **params)
        _, v = w.get_state()
        assert np.array_equal(_w(imp.vel[0]), _w(v)), k
        nonzero += int((imp.jn != 0).sum())
        w.step(every - 1, **params)
    return nonzero


@pytest.mark.parametrize("form", list(HASHED))
@pytest.mark.parametrize("name", ["flat1100", "pile14"])
def test_vel_is_the_qvel_of_the_next_step(rb, monkeypatch, name, form):
    code, env = HASHED[form]
    _setenv(monkeypatch, env)
    with rb.World(_scene(name), max_partners=32) as w:
        nonzero = _vel_is_next_qvel(w, 58 if name == "flat1100" else 0)
        st = w.stats()
    assert st["hashed_form"] == code, st
    assert nonzero > 0


def test_vel_is_the_qvel_of_the_next_step_in_the_tile_form(rb, oracle, monkeypatch):
    """cells_half with its touching pairs set moving (at rest every contact
    separates).  The tile run of 3 steps before the first query has a threshold
    above every penetration, so it skips every contact and the pairs still
    approach when the query and the step(1) that follows (the scene's threshold,
    0) solve them; that step continues in the tile form.  The second query sees
    the state after the bounce."""
    _setenv(monkeypatch, {"RBHIP_TILE": "1"})
    pb, _, _ = _case(oracle, ("world", "cells_half", "f64"), lambda: cg.make("cells_half"), "f64")
    sc = pb.scene(0)
    assert sc.threshold == 0.0
    v0 = np.zeros((pb.N, 6))
    v0[:, :3] = np.random.default_rng(21).uniform(-0.02, 0.02, (pb.N, 3))
    with rb.World(sc, max_partners=pb.max_partners) as w:
        w.set_state(pb.qpos, v0)
        nonzero = []
        for k, (run, thr) in enumerate(((3, 1.0), (2, 0.0))):
            w.step(run, threshold=thr)
            imp = w.query_impulses()
            w.step(1)
            _, v = w.get_state()
            assert np.array_equal(_w(imp.vel[0]), _w(v)), k
            nonzero.append(int((imp.jn != 0).sum()))
        st = w.stats()
    print(f"tile form: {nonzero} records with jn != 0 in the two queries")
    assert st["form"] == 5 and st["tile_rollbacks"] == 0 and st["tile_steps"] == 7, st
    assert nonzero[0] > 0


@pytest.mark.parametrize("how", ["host", "device"])
def test_applied_forces_are_honoured(rb, torch, how):
    sc = _scene("pile14")
    rng = np.random.default_rng(31)
    xfrc = rng.uniform(-0.5, 0.5, (sc.n, 6))
    xfrc[[2, 9]] = 0.0                                       # all-zero rows among them: the applied-force path all the same
    with rb.World(sc, max_partners=32) as w:
        free = w.query_impulses()
        if how == "host":
            w.set_xfrc(xfrc)
        else:
            w.set_xfrc_device(torch.from_numpy(xfrc).to("cuda:0"))
        forced = w.query_impulses()
        assert "vel" in differing(forced, free) and not differing(forced, free, RECORDS)
        assert np.array_equal(forced.vel[:, [2, 9]], free.vel[:, [2, 9]])    # (a zero row: at most the sign of a zero)
        nonzero = _vel_is_next_qvel(w, 0)
        assert nonzero > 0
        w.set_xfrc(None)                                     # forces cleared: the query follows
        q, v = w.get_state()
        ref, _ = model_dense(sc, q, v, free.max_records)
        assert not differing(w.query_impulses(), ref)


def test_the_parameters_of_the_call_count(rb, oracle):
    """Each of dt, restitution, friction and threshold, changed alone in the
    call: the query equals the model with that parameter, the model says vel
    changes, and the step with the same parameters writes that vel."""
    sc = _scene("pile14")
    with rb.World(sc, max_partners=32) as w:
        w.step(120)
        q, v = w.get_state()
        base = w.query_impulses()
        R = base.max_records
        ref0, m0 = model_dense(sc, q, v, R)
        assert not differing(base, ref0)
        pen = np.abs(m0.dist[m0.dist < 0])
        thr = float(np.median(pen))                          # skips the shallower half of the contacts
        changes = {"dt": sc.dt * 0.5, "restitution": sc.restitution * 0.5 + 0.11, "friction": sc.friction * 0.5 + 0.07,
                   "threshold": thr}
        assert all(value != getattr(sc, name) for name, value in changes.items())
        for name, value in changes.items():
            ref, m = model_dense(sc, q, v, R, **{name: value})
            assert not _same(ref["vel"], ref0["vel"]), name                # the model says it matters
            if name == "threshold":
                assert m.skipped > 0 and m.applied > 0
            got = w.query_impulses(**{name: value})
            assert not differing(got, ref), name
            assert not differing(got, base, RECORDS), name               # the list is the state's alone
        # all four at once, against the step
        w.step(1, **changes)
        _, v1 = w.get_state()
        w.set_state(q, v)
        got = w.query_impulses(**changes)
        assert np.array_equal(_w(got.vel[0]), _w(v1))


def test_the_raw_normal_convention(rb, oracle):
    sc = _scene("flat144")
    raw = sc.with_(normal_convention="raw")
    with rb.World(sc, max_partners=32, normal_convention="raw") as w, rb.World(sc, max_partners=32) as o:
        q, v = w.get_state()
        got, ori = w.query_impulses(), o.query_impulses()
        ref, m = model_dense(raw, q, v, got.max_records)
        assert m.applied > 0 and (m.partner >= 0).any()      # sphere pairs: the contacts whose normal the convention turns
        assert not differing(got, ref)
        assert not differing(got, ori, RECORDS) and "jn" in differing(got, ori)
        assert _vel_is_next_qvel(w, 0, queries=2) > 0


# ------------------------------------------------------------ 3. against the contact query
@pytest.mark.parametrize("name,steps", [("pile70", 40), ("flat1100", 60)])
def test_records_are_the_contact_querys(rb, name, steps):
    sc = _scene(name)
    with rb.World(sc, max_partners=32) as w:
        w.step(steps)
        for first, count, R in ((0, None, None), (0, None, 2), (5, sc.n - 11, 1), (sc.n - 1, 1, 8)):
            imp = w.query_impulses(first, count, max_records=R)
            con = w.query_contacts(first, count, max_records=imp.max_records, geometry=False)
            assert con.counts.sum() > 0 or count == 1
            assert not differing(imp, con, RECORDS), (first, count, R)
            assert imp.truncated == con.truncated and _fill_ok(imp)


# ------------------------------------------------------------ 4. ranges and truncation
def test_ranges_and_truncation(rb):
    sc = _scene("pile14")
    with rb.World(sc, max_partners=32) as w:
        w.step(120)
        full = w.query_impulses()
        assert full.counts.max() == 3
        for lo, hi in ((0, 1), (3, 11), (13, 14), (1, 14)):
            part = w.query_impulses(first=lo, count=hi - lo)
            assert part.first == lo and not differing(part, rows(full, lo, hi)), (lo, hi)
        for R in (0, 1, 8):
            cut = w.query_impulses(max_records=R)
            assert cut.max_records == R and not differing(cut, full, ("counts", "vel", "net")), R
            assert cut.truncated == int((full.counts > R).sum()) and (cut.truncated > 0) == (R < 3)
            if R == 0:
                assert all(getattr(cut, f) is None for f in ("partner", "kind", "dist", "jn", "jt"))
            else:
                for f in ("partner", "kind", "dist", "jn", "jt"):
                    assert _same(getattr(cut, f)[:, :, :min(R, 3)], getattr(full, f)[:, :, :min(R, 3)]), (R, f)
                assert _fill_ok(cut)
        # vel alone, net alone, through the raw binding
        p = rb._lib.ptr
        par = w._params(None, None, None, None)
        for which in ("vel", "net"):
            cnt, row = np.zeros(sc.n, np.int32), np.full((sc.n, 6), 7.5)
            rc = w._L.rb_query_impulses(w._h, 0, sc.n, 0, *par, p(cnt), None, None, None, None, None,
                                        p(row) if which == "vel" else None, p(row) if which == "net" else None, None)
            assert rc == 0, w._L.rb_last_error()
            assert _same(cnt[None], full.counts) and _same(row[None], getattr(full, which)), which


def test_host_form_in_sub_ranges_under_a_small_staging_bound(rb, monkeypatch):
    """A staging bound of 16 KiB cuts the 1,100 bodies into more than 30
    launches; a bound below one body's slots is RB_EINVAL."""
    sc = _scene("flat1100")
    with rb.World(sc, max_partners=32) as w:
        w.step(60)
        q, v = w.get_state()
        full = w.query_impulses(max_records=8)
    monkeypatch.setenv("RBHIP_CONTACT_STAGE_BYTES", str(16 << 10))
    per = 8 * (5 * 8 + 12) + 4 * (1 + 2 * 8)
    assert (16 << 10) // per < sc.n // 30
    with rb.World(sc, max_partners=32) as w:
        w.set_state(q, v)
        assert not differing(w.query_impulses(max_records=8), full)
        assert not differing(w.query_impulses(first=7, count=1000, max_records=8), rows(full, 7, 1007))
    monkeypatch.setenv("RBHIP_CONTACT_STAGE_BYTES", "256")
    with rb.World(sc, max_partners=32) as w:
        with pytest.raises(rb.RbError, match="EINVAL.*staging"):
            w.query_impulses(max_records=8)
        small = w.query_impulses()                           # (None: capped by the bound)
        assert 0 < small.max_records < 8


# ------------------------------------------------------------ 5. purity
def _interleave(rb, sc, q0, v0, runs, seed, max_partners):
    """Worlds A and B step the same runs; A is queried between them with both
    forms at random ranges and R (the pattern of test_gpu_world_contacts.py).
    After every run: the same state in uint64, the same stats key for key."""
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
                    imp = A.query_impulses(first, count, max_records=R, strict=False)
                    assert imp.counts.shape == (1, count) and imp.counts.min() >= 0
                else:                            # (enqueued only; the tensors live until the stream has run)
                    held.append(A.query_impulses_device(first, count, max_records=R))
                asked += 1
            A.step(k)
            B.step(k)
            held.clear()                         # (step() waited for the stream)
            qa, va = A.get_state()
            qb, vb = B.get_state()
            assert np.array_equal(_w(qa), _w(qb)) and np.array_equal(_w(va), _w(vb)), (r, k)
            sa, sb = A.stats(), B.stats()
            assert sa == sb, (r, {key: (sa[key], sb[key]) for key in sa if sa[key] != sb.get(key)})
        assert asked >= len(runs)
        return A.stats()


def _runs(rng, total=60, lo=1, hi=7):
    out = []
    while sum(out) < total:
        out.append(int(min(rng.integers(lo, hi + 1), total - sum(out))))
    if out[-1] < lo:                             # (the tile case: no run shorter than lo)
        last = out.pop()
        out[-1] += last
    return out


@pytest.mark.parametrize("form", list(HASHED))
@pytest.mark.parametrize("name", ["flat1100", "pile14"])
def test_queries_change_nothing_a_step_can_see(rb, torch, monkeypatch, name, form):
    code, env = HASHED[form]
    _setenv(monkeypatch, env)
    sc = _scene(name)
    runs = _runs(np.random.default_rng(41))
    assert sum(runs) == 60 and min(runs) >= 1 and max(runs) <= 7
    st = _interleave(rb, sc, sc.qpos0, sc.qvel0, runs, 42, 32)
    assert st["hashed_form"] == code, st


def test_queries_change_nothing_in_the_tile_form(rb, torch, oracle, monkeypatch):
    _setenv(monkeypatch, {"RBHIP_TILE": "1"})
    pb, _, _ = _case(oracle, ("world", "cells_half", "f64"), lambda: cg.make("cells_half"), "f64")
    runs = _runs(np.random.default_rng(43), lo=2)
    assert sum(runs) == 60 and min(runs) >= 2
    st = _interleave(rb, pb.scene(0), pb.qpos, np.zeros((pb.N, 6)), runs, 44, pb.max_partners)
    assert st["form"] == 5 and st["tile_rollbacks"] == 0 and st["tile_steps"] == 60, st


# ------------------------------------------------------------ 6. no list
def _host_imp(rb, dev):
    """A device query's arrays on the host, reals widened to double."""
    out = []
    for f in FIELDS:
        a = getattr(dev, f)
        a = None if a is None else a.cpu().numpy()
        out.append(a if a is None or a.dtype.kind != "f" else a.astype(np.float64))
    return rb.WorldImpulses(*out, None, dev.first)


def test_more_than_32_partners_is_a_body_without_a_list(rb, torch):
    import test_gpu_world_contacts as twc
    pb = twc._ring_scene()
    assert pb.N == 41
    rng = np.random.default_rng(51)
    v0 = rng.uniform(-0.1, 0.1, (pb.N, 6))
    with rb.World(pb.scene(0), max_partners=32) as w, rb.World(pb.scene(0), max_partners=32) as twin:
        w.set_state(pb.qpos, v0)
        twin.set_state(pb.qpos, v0)
        with pytest.raises(rb.RbError, match=r"EOVERFLOW.*body 0 ") as exc:
            w.query_impulses()
        assert exc.value.code == EOVERFLOW
        imp = w.query_impulses(strict=False)
        assert imp.counts[0, 0] == -2 and (imp.counts[0, 1:] == 1).all() and _fill_ok(imp) and imp.truncated == 0
        assert imp.kind[0, 0].tolist() == [-1] * imp.max_records
        assert not _w(imp.vel[0, 0]).any() and not _w(imp.net[0, 0]).any()
        assert imp.vel[0, 1:].any(axis=1).all()                          # the listed bodies have their rows
        con = w.query_contacts(strict=False, geometry=False)
        assert not differing(imp, con, RECORDS)
        dev = w.query_impulses_device(max_records=imp.max_records)
        w.sync()
        assert not differing(_host_imp(rb, dev), imp)
        # the world's error word was not touched: the queried world steps (or is refused) exactly as its twin
        outcomes = []
        for x in (w, twin):
            try:
                x.step(1)
                outcomes.append(("ok", 0))
            except rb.RbError as e:
                outcomes.append(("error", e.code))
        assert outcomes[0] == outcomes[1], outcomes
    # 30 touching partners: every body has a list, and the world still steps: vel is that step's qvel
    pb = twc._ring_scene(30)
    with rb.World(pb.scene(0), max_partners=32) as w:
        w.set_state(pb.qpos, v0[:31])
        imp = w.query_impulses()
        assert imp.counts[0].tolist() == [30] + [1] * 30
        w.step(1)
        assert np.array_equal(_w(imp.vel[0]), _w(w.get_state()[1]))


def test_a_nan_position_is_a_body_without_a_list(rb, torch):
    from rbhip import scenes
    sc = scenes.flat_spheres(8, 8)
    with rb.World(sc) as w:
        clean = w.query_impulses(max_records=4)
        q = sc.qpos0.copy()
        q[5, 0] = np.nan
        w.set_state(q, sc.qvel0)
        with pytest.raises(rb.RbError, match=r"EDOM.*body 5 ") as exc:
            w.query_impulses(max_records=4)
        assert exc.value.code == EDOM
        imp = w.query_impulses(max_records=4, strict=False)
        assert imp.counts[0, 5] == -2 and (np.delete(imp.counts[0], 5) >= 0).all() and _fill_ok(imp)
        assert not _w(imp.vel[0, 5]).any() and not _w(imp.net[0, 5]).any()
        assert not (clean.partner == 5).any()                # (no list of the clean state names body 5)
        keep = np.arange(sc.n) != 5
        assert not differing({f: getattr(imp, f)[:, keep] for f in FIELDS}, {f: getattr(clean, f)[:, keep] for f in FIELDS})
        dev = w.query_impulses_device(max_records=4)
        w.sync()
        assert not differing(_host_imp(rb, dev), imp)
        assert w.query_impulses(first=6, max_records=4).counts.min() >= 0    # a range that leaves the body out


# ------------------------------------------------------------ 7. the device form
def test_device_form_float32_outputs_are_the_c_cast(rb, torch):
    sc = _scene("pile14")
    with rb.World(sc, max_partners=32) as w:
        w.step(120)
        host = w.query_impulses(max_records=4)
        d64 = w.query_impulses_device(max_records=4)
        d32 = w.query_impulses_device(max_records=4, dtype="f32")
        sens = w.query_impulses_device(max_records=0, dtype="f32")
        w.sync()
        assert d64.truncated is None and d64.jn.dtype == torch.float64 and d32.jt.dtype == torch.float32
        assert not differing(_host_imp(rb, d64), host) and (host.jn != 0).any()
        for f in FIELDS:
            a32, a64 = getattr(d32, f).cpu().numpy(), getattr(d64, f).cpu().numpy()
            want = a64.astype(np.float32) if a64.dtype.kind == "f" else a64
            assert _same(a32, want), f
        assert sens.partner is None and sens.jn is None and sens.vel.dtype == torch.float32
        assert _same(sens.vel.cpu().numpy(), d32.vel.cpu().numpy()) and _same(sens.net.cpu().numpy(), d32.net.cpu().numpy())


def test_device_form_stream_order_and_out(rb, torch):
    sc = _scene("flat144")
    q0, v0 = sc.qpos0.copy(), sc.qvel0.copy()
    with rb.World(sc, max_partners=32) as ref:             # the host form, held to the model above
        ref.set_state(q0, v0)
        want0 = ref.query_impulses(max_records=4)
        ref.step(3)
        want3 = ref.query_impulses(max_records=4)
    assert (want0.jn != 0).any() and "vel" in differing(want3, want0)
    with rb.World(sc, max_partners=32) as w:
        w.set_stream(torch.cuda.current_stream().cuda_stream)
        dq, dv = torch.from_numpy(q0).to("cuda:0"), torch.from_numpy(v0).to("cuda:0")
        # nothing waits between these five
        w.set_state_device(dq, dv, refit=False)
        a = w.query_impulses_device(max_records=4)
        w.step_async(3)
        b = w.query_impulses_device(max_records=4)
        w.sync()
        assert not differing(_host_imp(rb, a), want0) and not differing(_host_imp(rb, b), want3)
        # out=: the given tensors are written and returned
        ptrs = {f: getattr(a, f).data_ptr() for f in FIELDS}
        for f in FIELDS:
            getattr(a, f).fill_(-3)
        again = w.query_impulses_device(out=a)
        w.sync()
        assert again.max_records == 4 and all(getattr(again, f).data_ptr() == ptrs[f] for f in FIELDS)
        assert not differing(_host_imp(rb, again), want3)
        with pytest.raises(ValueError, match="max_records"):
            w.query_impulses_device(max_records=8, out=a)
        with pytest.raises(ValueError, match="all five"):
            w.query_impulses_device(out={"counts": a.counts, "partner": a.partner, "kind": a.kind, "dist": a.dist})
        sensor = w.query_impulses_device(out={"counts": a.counts, "net": a.net})
        w.sync()
        assert sensor.partner is None and sensor.vel is None
        assert _same(sensor.net.cpu().numpy(), want3.net) and _same(sensor.counts.cpu().numpy(), want3.counts)


# ------------------------------------------------------------ 8. refusals
def test_refusals(rb, torch):
    from rbhip import scenes
    sc = scenes.flat_spheres(8, 8, spacing=0.19)
    N, R = sc.n, 4
    cnt, par, kin = np.zeros(N, np.int32), np.zeros((N, R), np.int32), np.zeros((N, R), np.int32)
    dis, jn, jt, row = np.zeros((N, R)), np.zeros((N, R)), np.zeros((N, R, 3)), np.zeros((N, 6))
    p = rb._lib.ptr
    d = {k: torch.zeros(s, dtype=t, device="cuda:0") for k, s, t in
         (("cnt", (N,), torch.int32), ("par", (N, R), torch.int32), ("kin", (N, R), torch.int32),
          ("dis", (N, R), torch.float64), ("jn", (N, R), torch.float64), ("jt", (N, R, 3), torch.float64),
          ("row", (N, 6), torch.float64))}
    dp = {k: C.c_void_p(v.data_ptr()) for k, v in d.items()}
    inf, nan = float("inf"), float("nan")
    with rb.World(sc) as w:
        w.step(30)
        L, h = w._L, w._h
        base = w.query_impulses(max_records=R)
        q0, v0 = w.get_state()
        st0 = w.stats()
        sdt, se, smu, sthr = w._params(None, None, None, None)

        def host(first=0, count=N, r=R, dt=sdt, e=se, mu=smu, thr=sthr, c=p(cnt), a=p(par), k=p(kin), x=p(dis), n=p(jn),
                 t=p(jt), v=p(row), s=None, hh=h):
            return L.rb_query_impulses(hh, first, count, r, dt, e, mu, thr, c, a, k, x, n, t, v, s, None)

        def dev(first=0, count=N, r=R, dt=sdt, e=se, mu=smu, thr=sthr, c=dp["cnt"], a=dp["par"], k=dp["kin"], x=dp["dis"],
                n=dp["jn"], t=dp["jt"], v=dp["row"], s=None, io=0, hh=h):
            return L.rb_query_impulses_dev(hh, first, count, r, dt, e, mu, thr, c, a, k, x, n, t, v, s, io)

        none5 = dict(a=None, k=None, x=None, n=None, t=None)
        refused = [
            ("null world", lambda f: f(hh=None)), ("counts", lambda f: f(c=None)), ("max_records < 0", lambda f: f(r=-1)),
            ("max_records 0", lambda f: f(r=0)), ("max_records 4", lambda f: f(**none5)),
            ("only all together", lambda f: f(k=None)), ("only all together", lambda f: f(n=None)),
            ("only all together", lambda f: f(t=None)), ("only all together", lambda f: f(r=0, a=None, k=None, x=None)),
            ("outside", lambda f: f(first=-1)), ("outside", lambda f: f(count=-1)), ("outside", lambda f: f(first=1)),
            ("outside", lambda f: f(first=N + 1, count=0)),
            # what rb_step refuses, and the non-finite values it would let through
            ("step parameters", lambda f: f(dt=0.0)), ("step parameters", lambda f: f(dt=-1e-3)),
            ("step parameters", lambda f: f(dt=nan)), ("step parameters", lambda f: f(e=-0.1)),
            ("step parameters", lambda f: f(mu=-0.1)), ("step parameters", lambda f: f(thr=-1e-9)),
            ("step parameters", lambda f: f(e=nan)), ("step parameters", lambda f: f(mu=nan)),
            ("step parameters", lambda f: f(thr=nan)),
            ("non-finite", lambda f: f(dt=inf)), ("non-finite", lambda f: f(e=inf)), ("non-finite", lambda f: f(mu=inf)),
            ("non-finite", lambda f: f(thr=inf)),
        ]
        for form in (host, dev):
            for text, call in refused:
                assert call(form) == EINVAL, (form.__name__, text)
                assert text.encode() in L.rb_last_error(), (form.__name__, text, L.rb_last_error())
        assert dev(io=7) == EINVAL and b"io_dtype" in L.rb_last_error()
        # a host pointer given to the device form
        for name, hostp in (("c", p(cnt)), ("a", p(par)), ("x", p(dis)), ("n", p(jn)), ("t", p(jt)), ("v", p(row)), ("s", p(row))):
            assert dev(**{name: hostp}) == EINVAL and b"not device memory" in L.rb_last_error(), name
        with pytest.raises(TypeError, match="counts"):
            w.query_impulses_device(out={"counts": cnt})
        w.sync()
        assert not any(t.any().item() for t in d.values())    # nothing was enqueued
        assert not cnt.any() and not row.any()
        for form in (host, dev):
            assert form(first=N, count=0) == 0 and form(first=3, count=0) == 0
            assert form(r=0, **none5) == 0 and form(r=0, v=None, **none5) == 0      # the sensor-only call; vel left out
        w.sync()
        assert not differing(w.query_impulses(max_records=R), base)
        assert all(np.array_equal(_w(a), _w(b)) for a, b in zip(w.get_state(), (q0, v0)))
        assert w.stats() == st0
    with rb.World(sc, rank=0, world_size=2) as w:
        par5 = w._params(None, None, None, None)
        assert w._L.rb_query_impulses(w._h, 0, 1, 0, *par5, p(cnt), None, None, None, None, None, None, None, None) == EUNSUPPORTED
        assert b"world_size" in w._L.rb_last_error()
        assert w._L.rb_query_impulses_dev(w._h, 0, 1, 0, *par5, dp["cnt"], None, None, None, None, None, None, None, 0) == EUNSUPPORTED
        with pytest.raises(rb.RbError, match="EUNSUPPORTED"):
            w.query_impulses()
    with rb.World(scenes.ball_collision(), law="balls") as w:
        with pytest.raises(rb.RbError, match="EUNSUPPORTED.*two-ball"):
            w.query_impulses()
        with pytest.raises(rb.RbError, match="EUNSUPPORTED"):
            w.query_impulses_device(max_records=0)


def test_device_form_is_refused_under_a_stream_capture(rb, torch):
    from rbhip import scenes
    sc = scenes.flat_spheres(8, 8, spacing=0.19)
    with rb.World(sc) as w:
        w.step(30)
        base = w.query_impulses(max_records=0)
        cnt = torch.zeros(sc.n, dtype=torch.int32, device="cuda:0")
        vel = torch.zeros((sc.n, 6), dtype=torch.float64, device="cuda:0")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        w.set_stream(s.cuda_stream)
        g = torch.cuda.CUDAGraph()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)     # (torch remarks that the captured graph is empty: it is)
            with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                rc = w._L.rb_query_impulses_dev(w._h, 0, sc.n, 0, *w._params(None, None, None, None),
                                                C.c_void_p(cnt.data_ptr()), None, None, None, None, None,
                                                C.c_void_p(vel.data_ptr()), None, 0)
                msg = w._L.rb_last_error()
        w.set_stream(0)
        assert rc == EUNSUPPORTED and b"capture" in msg, (rc, msg)
        torch.cuda.synchronize()
        assert not cnt.any().item() and not vel.any().item()  # nothing was enqueued, nothing captured
        assert not differing(w.query_impulses(max_records=0), base)
