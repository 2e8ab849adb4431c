"""The wide + helper form with the contact search shared between its two
waves: the body lane of a body searches the four buckets on
its own side of the split axis, the helper lane the four on the neighbour
side; the body wave merges the two hit lists and sorts them by id.

Bar: contacts, contact order and state are what the oracle computes, bit for
bit.  Every test forces the form at small sizes (RBHIP_COOP_MAX_BODIES=0,
RBHIP_WIDE_HELP=1) and checks hashed_form == 4 and the help_search counter."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the axis the search is split along (rb_grid.hpp RB_SHARE_AXIS): a partner
# whose cell coordinate on it differs from the body's is in the helper's half
SPLIT_AXIS = 1


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


def _same(a, b):
    """Bit identity as 64-bit words (the sign of zeros counts)."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _form(monkeypatch, epoch=None, share=True, **env):
    monkeypatch.setenv("RBHIP_COOP_MAX_BODIES", "0")
    monkeypatch.setenv("RBHIP_WIDE_HELP", "1")
    monkeypatch.setenv("RBHIP_HELP_SEARCH", "1" if share else "0")
    if epoch is not None:
        monkeypatch.setenv("RBHIP_TABLE_EPOCH", str(epoch))
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _check_form(st, share=True):
    assert st["hashed_form"] == 4, st
    assert st["help_search"] == (1 if share else 0), st


def _cells(sc, q):
    cs = 4.0 * float(sc.size[:, 0].max()) * 1.001
    return np.floor(q.reshape(-1, 7)[:, :3] / cs).astype(np.int64)


def _half_counts(sc, q_start, cnt, par, kin):
    """Per body, from one step's oracle lists and step-start positions: the
    sphere partners in the body wave's half and in the helper's, and whether
    a helper-half partner sorts before a body-half one."""
    c = _cells(sc, q_start)[:, SPLIT_AXIS]
    body = np.repeat(np.arange(sc.n), cnt)
    m = kin == 16
    b, p = body[m], par[m]
    other = c[p] != c[b]
    na = np.bincount(b[~other], minlength=sc.n)
    nb = np.bincount(b[other], minlength=sc.n)
    max_a = np.full(sc.n, -1, np.int64)
    min_b = np.full(sc.n, np.iinfo(np.int64).max, np.int64)
    np.maximum.at(max_a, b[~other], p[~other])
    np.minimum.at(min_b, b[other], p[other])
    return na, nb, (na > 0) & (nb > 0) & (min_b < max_a)


_crowd = {}


def _crowded_reference(oracle):
    """flat_spheres(33, 31, seed=5, spacing=0.15): the oracle's 200 recorded
    steps from t = 0 (computed once; arrays read-only)."""
    if not _crowd:
        from rbhip import scenes
        sc = scenes.flat_spheres(33, 31, seed=5, spacing=0.15)
        osc = oracle.OracleScene(sc)
        q, v = sc.qpos0, sc.qvel0
        steps, both, inter, longest = [], 0, 0, 0
        for _ in range(200):
            q0 = q
            q, v, (cnt, par, kin, dis) = oracle.step(osc, q, v, 1, record=True)
            na, nb, mixed = _half_counts(sc, q0, cnt, par, kin)
            both += int(((na > 0) & (nb > 0)).sum())
            inter += int(mixed.sum())
            longest = max(longest, int((na + nb).max()))
            for a in (cnt, par, kin, dis):
                a.setflags(write=False)
            steps.append((cnt, par, kin, dis))
        q.setflags(write=False)
        v.setflags(write=False)
        _crowd.update(sc=sc, steps=steps, q=q, v=v, both=both, inter=inter, longest=longest)
    return _crowd


@pytest.mark.parametrize("epoch", [1, 8])
def test_merge_order_across_the_halves(rb, oracle, monkeypatch, epoch):
    """1,023 bodies (the last wave has 63 lanes), 200 single recorded steps
    from t = 0: per step the contact counts, partners, kinds and distances
    equal the oracle's, and the final state is identical.  From the oracle's
    lists: at least 200 body-steps have sphere partners in both halves of the
    split, and in at least 100 of them a helper-half partner sorts before a
    body-half one."""
    ref = _crowded_reference(oracle)
    print(f"body-steps with partners in both halves {ref['both']}, of which interleaved {ref['inter']}, "
          f"longest list {ref['longest']}")
    assert ref["both"] >= 200 and ref["inter"] >= 100
    _form(monkeypatch, epoch)
    sc = ref["sc"]
    assert sc.n == 1023
    with rb.World(sc) as w:
        w.record_contacts(True)
        for t, (cnt, par, kin, dis) in enumerate(ref["steps"]):
            w.step(1)
            gc, gp, gk, gd = w.contacts()
            assert np.array_equal(gc, cnt), f"contact counts differ at step {t}"
            assert np.array_equal(gp, par) and np.array_equal(gk, kin), f"partners / kinds differ at step {t}"
            assert _same(gd, dis), f"contact distances differ at step {t}"
        q, v = w.get_state()
        st = w.stats()
    _check_form(st)
    assert st["table_epoch"] == epoch, st
    assert (st["append_steps"] > 0) == (epoch > 1), st
    assert _same(q, ref["q"]) and _same(v, ref["v"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rare_path_in_both_halves(rb, oracle, monkeypatch, dtype):
    """The crowded-cell bar of the wide form (cells of 7+ bodies: ids past a
    bucket head's 6) through the shared search: 120 graph-replayed steps,
    then one recorded step, contacts and state bit-exact with the oracle."""
    from rbhip import scenes
    _form(monkeypatch)
    sc = scenes.flat_spheres(33, 31, seed=5, spacing=0.15)
    osc = oracle.OracleScene(sc)
    q0, v0 = oracle.step(osc, sc.qpos0, sc.qvel0, 120, dtype=dtype)
    q1, v1, (cnt, par, kin, dis) = oracle.step(osc, q0, v0, 1, dtype=dtype, record=True)
    with rb.World(sc, dtype=dtype) as w:
        w.step(120)
        w.record_contacts(True)
        w.step(1)
        q, v = w.get_state()
        gc, gp, gk, gd = w.contacts()
        st = w.stats()
    _check_form(st)
    assert np.array_equal(gc, cnt) and np.array_equal(gp, par) and np.array_equal(gk, kin)
    assert _same(gd, dis)
    assert _same(q, q1) and _same(v, v1)
    # cells (2 x 2 r = 0.4 m) holding 7+ bodies, and partners in both halves of such bodies' lists
    cells = np.floor(q0.reshape(-1, 7)[:, :3] / 0.4).astype(np.int64)
    _, per_cell = np.unique(cells, axis=0, return_counts=True)
    assert per_cell.max() >= 7
    na, nb, _ = _half_counts(sc, q0, cnt, par, kin)
    assert ((na > 0) & (nb > 0)).sum() > 0
    # ... and a cell of 7+ bodies among the four cells of some body's helper half
    cs = 4.0 * float(sc.size[:, 0].max()) * 1.001
    f = q0.reshape(-1, 7)[:, :3] / cs
    c0 = np.floor(f).astype(np.int64)
    side = np.where(f - c0 < 0.5, -1, 1)
    crowd = {tuple(c) for c, k in zip(*np.unique(c0, axis=0, return_counts=True)) if k >= 7}
    ax = [a for a in range(3) if a != SPLIT_AXIS]
    helper_crowded = 0
    for c, sg in zip(c0, side):
        for da in (0, 1):
            for db in (0, 1):
                n = c.copy()
                n[SPLIT_AXIS] += sg[SPLIT_AXIS]
                n[ax[0]] += da * sg[ax[0]]
                n[ax[1]] += db * sg[ax[1]]
                helper_crowded += tuple(n) in crowd
    assert helper_crowded > 0


def test_ragged_and_packed_shared_and_not(rb, oracle, monkeypatch):
    """1,073 bodies on a packed grid (spacing 0.19 < 2r), 121 steps, with the
    shared search on and off, as one step(121) graph and as single launches:
    every run identical to the oracle, hence to each other."""
    from rbhip import scenes
    sc = scenes.flat_spheres(37, 29, spacing=0.19)
    assert sc.n == 1073
    q0, v0 = oracle.step(oracle.OracleScene(sc), sc.qpos0, sc.qvel0, 121)
    runs = {}
    for share in (True, False):
        _form(monkeypatch, share=share)
        for mode in ("graph", "single"):
            with rb.World(sc) as w:
                if mode == "graph":
                    w.step(121)
                else:
                    for _ in range(121):
                        w.step_async(1)
                    w.sync()
                runs[share, mode] = w.get_state()
                _check_form(w.stats(), share)
    for key, (q, v) in runs.items():
        assert _same(q, q0) and _same(v, v0), f"shared search {key[0]}, {key[1]}: state differs from the oracle"
    qa, va = runs[True, "graph"]
    for q, v in runs.values():
        assert _same(q, qa) and _same(v, va)


@pytest.mark.parametrize("axis,env,grid", [
    ("z", {"RBHIP_HASH_GROUP": "5:5:0"}, (16, 16, 0.3)),
    ("y", {"RBHIP_HASH_GROUP": "5:0:5", "RBHIP_HASH_PERIOD": "2:0:0"}, (48, 3, 0.17)),
])
def test_visit_once_under_folding(rb, oracle, monkeypatch, axis, env, grid):
    """A table of 4,096 buckets whose period is one cell along one axis
    (groups one cell thick there and no period bit for it: RBHIP_HASH_GROUP,
    RBHIP_HASH_FACTOR, RBHIP_HASH_PERIOD, the creation-time period kept), so
    the two layers of every body's neighbourhood along that axis fold onto
    the same four buckets; the layout is read back from the world.  Along z
    both buckets of a folded pair belong to one wave.  Along y, the split
    axis, every bucket of the helper's half equals one of the body wave's
    half: the helper must list none of them, or every contact shows twice.
    (The period fit never folds y on its own — the y neighbours of occupied
    groups would collide with them — hence the explicit period.)  100 steps,
    then 20 recorded ones, contacts and state against the oracle, with at
    least 50 sphere-sphere contacts in the recorded steps."""
    from rbhip import scenes
    _form(monkeypatch, RBHIP_HASH_FACTOR="4", RBHIP_FIT_PERIOD="0", **env)
    nx, ny, spacing = grid
    sc = scenes.flat_spheres(nx, ny, seed=2, spacing=spacing)
    osc = oracle.OracleScene(sc)
    q1, v1 = oracle.step(osc, sc.qpos0, sc.qvel0, 100)
    pairs = 0
    with rb.World(sc) as w:
        lay = w.stats()["grid_layout"]
        w.step(100)
        w.record_contacts(True)
        for t in range(20):
            q1, v1, (cnt, par, kin, dis) = oracle.step(osc, q1, v1, 1, record=True)
            w.step(1)
            gc, gp, gk, gd = w.contacts()
            assert np.array_equal(gc, cnt), f"contact counts differ at recorded step {t}"
            assert np.array_equal(gp, par) and np.array_equal(gk, kin), f"partners / kinds differ at recorded step {t}"
            assert _same(gd, dis), f"contact distances differ at recorded step {t}"
            pairs += int((kin == 16).sum())
        q, v = w.get_state()
        st = w.stats()
    _check_form(st)
    d = {"x": 0, "y": 1, "z": 2}[axis]
    # linear layout; groups one cell thick and a period of one group along the axis
    assert (lay >> 24) & 1 and (lay >> (4 * d)) & 15 == 0 and (lay >> (12 + 4 * d)) & 15 == 0, hex(lay)
    assert st["grid_layout"] == lay and st["refits"] == 0 and st["buckets"] == 4096, st
    assert _same(q, q1) and _same(v, v1)
    assert pairs >= 50                                 # sphere-sphere contacts in the recorded steps


def test_box_world_keeps_the_old_path_and_agrees_when_forced(rb, oracle, monkeypatch):
    """Worlds with boxes do not share the search by default (cubes measured
    slower with it).  Forced on, a body with a box-involved candidate in
    either half is deferred to the box kernel (the flag crosses the waves):
    tilted cube columns with sphere caps, 200 steps then 20 recorded ones,
    contacts and state bit-exact with the oracle."""
    from rbhip import scenes
    sc = scenes.box_pile(6, 6, 3, seed=0)
    _form(monkeypatch)
    monkeypatch.delenv("RBHIP_HELP_SEARCH")
    with rb.World(sc, max_partners=32) as w:
        st = w.stats()
        assert st["hashed_form"] == 4 and st["help_search"] == 0, st
    _form(monkeypatch)
    osc = oracle.OracleScene(sc, max_partners=32)
    q, v = oracle.step(osc, sc.qpos0, sc.qvel0, 200)
    seen = set()
    with rb.World(sc, max_partners=32) as w:
        w.step(200)
        gq, gv = w.get_state()
        assert _same(gq, q) and _same(gv, v)
        w.record_contacts(True)
        for s in range(20):
            q, v, (cnt, par, kin, dis) = oracle.step(osc, q, v, 1, record=True)
            w.step(1)
            gc, gp, gk, gd = w.contacts()
            assert np.array_equal(gc, cnt), f"contact counts differ at recorded step {s}"
            assert np.array_equal(gp, par) and np.array_equal(gk, kin), f"partners / kinds differ at recorded step {s}"
            assert _same(gd, dis), f"contact distances differ at recorded step {s}"
            seen |= set(kin.tolist())
        gq, gv = w.get_state()
        st = w.stats()
    _check_form(st)
    assert _same(gq, q) and _same(gv, v)
    assert any(k > 16 for k in seen), seen              # box-involved contacts in the recorded steps


# 2,048 spheres sliding down the incline pile into each other: the oracle's
# first lists of more than 16 partners are those of steps 657 and 658
_PILE = dict(nx=8, ny=256, spacing=0.3, steps=658)


def test_partner_overflow_across_the_halves(rb, oracle, monkeypatch):
    """A pile on the incline in which a body's partners pass 16 only as the
    sum of the two halves (asserted from the oracle's lists): the guarded
    synchronous chunk rolls back, raises max_partners to 32 and ends
    bit-exact with the oracle."""
    from rbhip import scenes
    _form(monkeypatch)
    sc = scenes.incline_spheres(_PILE["nx"], _PILE["ny"], seed=0, spacing=_PILE["spacing"])
    osc = oracle.OracleScene(sc, max_partners=32)
    oracle.set_threads(8)
    try:
        q, v = sc.qpos0, sc.qvel0
        over = 0
        for _ in range(_PILE["steps"]):
            qs = q
            q, v, (cnt, par, kin, dis) = oracle.step(osc, q, v, 1, record=True)
            na, nb, _ = _half_counts(sc, qs, cnt, par, kin)
            over += int(((na + nb > 16) & (na <= 16) & (nb <= 16)).sum())
            assert not ((na > 16) | (nb > 16)).any(), "a half alone passes 16 partners"
    finally:
        oracle.set_threads(1)
    assert over > 0, "no body passes 16 partners"
    with rb.World(sc) as w:
        assert w.stats()["max_partners"] == 16
        w.step(_PILE["steps"])
        gq, gv = w.get_state()
        st = w.stats()
    _check_form(st)
    assert st["max_partners"] == 32, st
    assert _same(gq, q) and _same(gv, v)
