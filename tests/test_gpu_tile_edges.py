"""The tile form's own code paths (csrc/rb_tiles.hip, rb_api_tiles.hip; DESIGN
§4.1) on small directed scenes: every tile width, both partner capacities,
both register sizings, the ring, the far list, the fold, the pile path, and
every failure reason raised on purpose.  Every case has at most 10,000 bodies
and 100 steps; is compared with the oracle bit for bit (the state as uint64
words, and where contacts are recorded their counts, partners, kinds and
distances); and asserts from stats() that it ran, or failed, in the tile form
as intended: the form, the steps committed, the roll-backs, the reason bits,
and the grid, which must be the one tests/tile_fit.py's mirror of the fit
gives.  tests/test_tile_fit.py shows on the CPU, from the mirror and the
oracle's trajectory, that each scene reaches the path it is meant to reach.

RBHIP_TILE_COLS is read at the fit (the first tile build and every refit),
not at world creation, so the tests keep it set until the steps have run.

The failure cases are roll-backs the library handles: the run is replayed by
the hashed forms from the state at its start, and must leave the oracle's
bits.

The tests can fail.  Five mutants of rb_tiles.hip, each changing a decision
or a read inside bounds, built apart from the tree and never committed
(DESIGN §4.1 has the same table), each run against the 48 new GPU tests
(these and test_gpu_contact_geometry.py's test_world_tile_family*) and against
15 earlier tile tests (test_gpu_tiles.py without its 1M-body and 2,000-step
cases, test_world_tile_form*):

  mutant                               new tests failing; earlier ones
  side switch frx >= T(0.5) -> >       none, rightly: the two differ only at
                                       frx = 0.5 exactly, where a partner (at
                                       most 2 rmax = 0.4995 columns away) lies
                                       in the body's own column, which both
                                       sides search: an equivalent mutant
  far-window admission vx > TC         test_ring_and_far_list_directed (both):
    -> vx >= TC                        the target in a tile's east column has
                                       no record of the mover that landed,
                                       through the far list, in the ring column
                                       east of it; earlier: none
  pile loop rr < WR -> rr <= WR        17: piles, fold, window_full_of_records,
                                       the families sheet_negative, _period,
                                       _radius, _piles at every width, 3 in
                                       fp32; earlier: 4
  tile_place pmod(tx, ntx)             40 (every scene with bodies at negative
    -> tx % ntx clamped to >= 0        tile indices); earlier: 7
  col_sources vx >= TC - 1 -> vx >= TC test_every_instantiation[tc5-*] (2), and
    in the TC = 5 instantiation only   no other; earlier: none (none runs TC 5)

What catches the far-window mutant: a resting target's own state does not
show a missed partner (the per-body law gives it no impulse at zero velocity),
and the mover is stepped by its own slot, so the ring test compares the
records of the run's second step, and four of its movers arrive through the
far list in a ring column of their target's window, one per side.
"""
import numpy as np
import pytest

import contact_geometry as cg
import tile_fit as tf

pytestmark = pytest.mark.gpu

EDOM = -33


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


@pytest.fixture
def oracle16(oracle):
    oracle.set_threads(16)
    yield oracle
    oracle.set_threads(1)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _world(rb, monkeypatch, sc, tile=1, cols=None, **kw):
    """A world created under RBHIP_TILE=tile (None: the default, auto);
    RBHIP_TILE_COLS stays set for the steps (the caller's monkeypatch undoes it)."""
    if tile is None:
        monkeypatch.delenv("RBHIP_TILE", raising=False)
    else:
        monkeypatch.setenv("RBHIP_TILE", str(tile))
    if cols is None:
        monkeypatch.delenv("RBHIP_TILE_COLS", raising=False)
    else:
        monkeypatch.setenv("RBHIP_TILE_COLS", str(cols))
    w = rb.World(sc, **kw)
    monkeypatch.delenv("RBHIP_TILE", raising=False)
    return w


def _state_is(w, q, v, what):
    gq, gv = w.get_state()
    assert _same(gq, q) and _same(gv, v), f"state differs {what}"


def _recorded_steps(w, oracle, osc, q, v, n, dtype="f64", what=""):
    """n single steps with contacts recorded, each equal to the oracle's."""
    w.record_contacts(True)
    for t in range(n):
        q, v, (cnt, par, kin, dis) = oracle.step(osc, q, v, 1, dtype=dtype, record=True)
        w.step(1)
        gc, gp, gk, gd = w.contacts()
        assert np.array_equal(gc, cnt), f"{what}: contact counts differ at recorded step {t}"
        assert np.array_equal(gp, par) and np.array_equal(gk, kin), f"{what}: partners differ at recorded step {t}"
        assert _same(gd, dis), f"{what}: contact distances differ at recorded step {t}"
        _state_is(w, q, v, f"after recorded step {t} ({what})")
    return q, v, kin


def _grid_is(st, fit):
    assert st["tile_cols"] == fit.tc and st["tile_slots"] == fit.slots, (st, fit)


def _committed(st, steps):
    assert st["form"] == tf.FORM_TILE and st["tile_steps"] == steps and st["tile_rollbacks"] == 0 \
        and st["tile_why"] == 0, st


# ------------------------------------------------------------ every instantiation
# (tc, max_partners, dtype): every width in both precisions and with both partner capacities
INSTANCES = [(tc, 16, "f64") for tc in cg.SHEET_TC] + [(tc, 32, "f32") for tc in cg.SHEET_TC] + \
            [(8, 32, "f64"), (6, 32, "f64"), (4, 16, "f32"), (7, 16, "f32")]


@pytest.mark.parametrize("tc,maxp,dtype", INSTANCES, ids=[f"tc{t}-maxp{m}-{d}" for t, m, d in INSTANCES])
def test_every_instantiation(rb, oracle16, monkeypatch, tc, maxp, dtype):
    """tile_step_kernel<T, MAXP, TC, 2> for every TC, both MAXP and both T:
    2,304 falling, colliding spheres, 60 steps as one graph run, then three
    single recorded steps."""
    sc = tf.falling_grid()
    fit = tf.fit(sc.qpos0, tf.COL, force=tc)
    assert fit.tc == tc and fit.slots <= tf.OCC3_SLOTS
    osc = oracle16.OracleScene(sc, max_partners=maxp)
    q, v = oracle16.step(osc, sc.qpos0, sc.qvel0, 60, dtype=dtype)
    with _world(rb, monkeypatch, sc, cols=tc, dtype=dtype, max_partners=maxp) as w:
        w.step(60)
        _state_is(w, q, v, "after 60 steps")
        q, v, kin = _recorded_steps(w, oracle16, osc, q, v, 3, dtype, f"tc {tc}")
        st = w.stats()
    assert (kin == 16).sum() > 0
    _committed(st, 63)
    _grid_is(st, fit)
    assert st["max_partners"] == maxp, st


# ------------------------------------------------------------ ring and far list
@pytest.mark.parametrize("tile0", [(2, 2), (-9, -8)], ids=["positive", "negative"])
def test_ring_and_far_list_directed(rb, oracle16, monkeypatch, tile0):
    """tile_fit.ring_movers: from the corner and edge columns of a tile a mover
    for every column displacement in {-2 .. 2}^2, each arriving on a resting
    target: the step after, the pair is a contact whose one side came through
    the ring (one column out) or the far list (two); four more arrive through
    the far list in a ring column of their target's window.  A run of 2 steps
    whose second is recorded (a resting target's own state does not show a
    missed partner: its record does), then 3 recorded single steps, every one
    committed."""
    sc, start, disp, ids = tf.ring_movers(tc=4, tile0=tile0)
    fit = tf.fit(sc.qpos0, tf.COL, force=4)
    osc = oracle16.OracleScene(sc)
    q, v = oracle16.step(osc, sc.qpos0, sc.qvel0, 1)
    q, v, (cnt, par, kin, dis) = oracle16.step(osc, q, v, 1, record=True)
    assert (cnt[ids + 1] == 1).all() and cnt.sum() == 2 * len(ids) + 8
    with _world(rb, monkeypatch, sc, cols=4) as w:
        w.record_contacts(True)
        w.step(2)
        gc, gp, gk, gd = w.contacts()
        assert np.array_equal(gc, cnt), f"contact counts differ at step 2: bodies {np.flatnonzero(gc != cnt)[:8]}"
        assert np.array_equal(gp, par) and np.array_equal(gk, kin) and _same(gd, dis)
        _state_is(w, q, v, "after 2 steps")
        q, v, kin = _recorded_steps(w, oracle16, osc, q, v, 3, what="ring")
        st = w.stats()
    _committed(st, 5)
    _grid_is(st, fit)


# ------------------------------------------------------------ the far list, committed
def test_far_list_committed(rb, oracle16, monkeypatch):
    """test_gpu_tiles.py's far movers at a quarter of the size: 6 of 1,024
    spheres cross up to 10 columns a step for 40 steps, and every step is
    committed in tile slots: the far list's scan, its generation tag, the
    far bodies' own step and the unbin kernel's far loop leave the oracle's
    bits."""
    sc, who = tf.far_movers()
    fit = tf.fit(sc.qpos0, tf.COL)
    osc = oracle16.OracleScene(sc)
    q, v = oracle16.step(osc, sc.qpos0, sc.qvel0, 37)
    with _world(rb, monkeypatch, sc) as w:
        w.step(37)
        _state_is(w, q, v, "after 37 steps")
        _recorded_steps(w, oracle16, osc, q, v, 3, what="far movers")
        st = w.stats()
    _committed(st, 40)
    _grid_is(st, fit)


# ------------------------------------------------------------ the fold, OCC 3, piles
def test_fold_while_stepping(rb, oracle16, monkeypatch):
    """Two falling patches of 1,024 spheres 654 m apart: the grid folds and
    tiles of both patches share slots for 60 steps and 3 recorded ones."""
    sc = tf.fold_patches()
    fit = tf.fit(sc.qpos0, tf.COL, force=4)
    assert fit.folded and fit.aliased >= 24
    osc = oracle16.OracleScene(sc)
    q, v = oracle16.step(osc, sc.qpos0, sc.qvel0, 60)
    with _world(rb, monkeypatch, sc, cols=4) as w:
        w.step(60)
        _state_is(w, q, v, "after 60 steps")
        _recorded_steps(w, oracle16, osc, q, v, 3, what="fold")
        st = w.stats()
    _committed(st, 63)
    _grid_is(st, fit)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_three_wave_kernel(rb, oracle16, monkeypatch, dtype):
    """tile_step_kernel<T, 16, 4, 3>: 8,100 sparse spheres on 33 x 33 slots of
    width 4 (more than 1,024, unfolded), 40 steps and 3 recorded ones."""
    sc = tf.sparse_grid()
    fit = tf.fit(sc.qpos0, tf.COL, force=4)
    assert fit.slots > tf.OCC3_SLOTS and not fit.folded
    osc = oracle16.OracleScene(sc)
    q, v = oracle16.step(osc, sc.qpos0, sc.qvel0, 40, dtype=dtype)
    with _world(rb, monkeypatch, sc, cols=4, dtype=dtype) as w:
        w.step(40)
        _state_is(w, q, v, "after 40 steps")
        _recorded_steps(w, oracle16, osc, q, v, 3, dtype, "three waves")
        st = w.stats()
    _committed(st, 43)
    _grid_is(st, fit)


def test_piles_while_stepping(rb, oracle16, monkeypatch):
    """tile_fit.falling_piles: stacks of 7 to 20 spheres under gravity for 40
    steps and 3 recorded ones: window columns of up to 32 records (the pile
    path).  The stacks only move vertically; 24 sliders pass over them one
    column a step, so from the second step on a pile column is read from two
    bins, a stack's and the ring of the sliders' tile (shown on the CPU:
    test_tile_fit.py).  The mirror on the oracle's states shows no slot past
    128 bodies and no window past 384 records there, so no roll-back is due."""
    sc, _ = tf.falling_piles()
    fit = tf.fit(sc.qpos0, tf.COL)
    osc = oracle16.OracleScene(sc)
    q, v = oracle16.step(osc, sc.qpos0, sc.qvel0, 40)
    with _world(rb, monkeypatch, sc) as w:
        w.step(40)
        _state_is(w, q, v, "after 40 steps")
        _recorded_steps(w, oracle16, osc, q, v, 3, what="piles")
        st = w.stats()
    _committed(st, 43)
    _grid_is(st, fit)


# ------------------------------------------------------------ every failure reason
def _after_failure(oracle, osc, w, q, v, st, why, tiled_steps=0, again=False):
    """The run was rolled back once for `why` and replayed bit-exact; two
    recorded steps and two further runs of 2 steps follow the oracle.  The
    first of those runs is the back-off's (hashed), the second is in the tile
    form again: it commits, or (again: the scene still does what made the
    first run fail) rolls back for the same reason and is replayed.  Returns
    the last state and the one the last run started at."""
    assert st["tile_rollbacks"] == 1 and st["tile_why"] & why and st["tile_steps"] == tiled_steps, st
    _state_is(w, q, v, "after the replay")
    q, v, _ = _recorded_steps(w, oracle, osc, q, v, 2, what="after the replay")
    for k in range(2):
        before = q
        q, v = oracle.step(osc, q, v, 2)
        w.step(2)
        _state_is(w, q, v, f"after further run {k}")
        now = w.stats()
        assert now["tile_runs"] == st["tile_runs"] + k, (k, now)
    if again:
        assert now["tile_rollbacks"] == 2 and now["tile_steps"] == tiled_steps and now["tile_why"] & why, now
    else:
        assert now["tile_rollbacks"] == 1 and now["tile_steps"] == tiled_steps + 2 and now["form"] == tf.FORM_TILE, now
    return q, v, before


def test_window_full_of_records(rb, oracle16, monkeypatch):
    """TILE_WHY_WINDOW, first cause: at width 8 every tile holds at most 104
    bodies, and the window of tile (0, 0), whose ring the four neighbours'
    stacks fill, 420 records.  Once RBHIP_TILE_COLS is gone the refit picks
    width 4 and the tile form commits."""
    sc = tf.window_stacks()
    fit = tf.fit(sc.qpos0, tf.COL, force=8)
    assert fit.tc == 8 and fit.worst_slot <= tf.FIT_MAX and fit.worst_window > tf.WMAX
    osc = oracle16.OracleScene(sc)
    q, v = oracle16.step(osc, sc.qpos0, sc.qvel0, 4)
    with _world(rb, monkeypatch, sc, cols=8) as w:
        w.step(4)
        st = w.stats()
        assert st["tile_why"] == tf.WHY["WINDOW"] and st["tile_cols"] == 8, st
        monkeypatch.delenv("RBHIP_TILE_COLS")
        q, v, before = _after_failure(oracle16, osc, w, q, v, st, tf.WHY["WINDOW"])
        st = w.stats()
    free = tf.fit(before, tf.COL)                       # (the refit: from the state the last run started at)
    assert free.tc == 4 and tf.holds(free), free
    _grid_is(st, free)


def test_window_full_of_far_bodies_in_a_chain(rb, oracle16, monkeypatch):
    """TILE_WHY_WINDOW, second cause, in the second of three chained async
    runs: tile_fit.far_throw's 40 movers are on the far list after every step
    and all stand over one column after step 4, so step 5 finds more than 32
    far bodies in one window.  The first run (2 steps) is committed and
    counted, the second (4) and the third (2) are replayed."""
    sc = tf.far_throw()
    osc = oracle16.OracleScene(sc)
    q, v = oracle16.step(osc, sc.qpos0, sc.qvel0, 8)
    with _world(rb, monkeypatch, sc, cols=4) as w:
        for n in (2, 4, 2):
            w.step_async(n)
        w.sync()
        st = w.stats()
        assert st["tile_why"] == tf.WHY["WINDOW"] and st["tile_runs"] == 3, st
        # the tile run after the back-off (steps 13 and 14, refitted from the state after 12) commits: the
        # movers have spread out again, at most 32 of them stand in one window when the far list is scanned
        q12, v12 = oracle16.step(osc, q, v, 4)
        q13, _ = oracle16.step(osc, q12, v12, 1)
        fit = tf.fit(q12, tf.COL, force=4)
        movers = np.arange(sc.n - 40, sc.n)
        assert tf.holds(fit) and tf.holds(tf.refit(fit, q13, tf.COL)), fit
        assert tf.refit(fit, q13[movers], tf.COL).worst_window <= tf.FARWIN
        _after_failure(oracle16, osc, w, q, v, st, tf.WHY["WINDOW"], tiled_steps=2)
        _grid_is(w.stats(), fit)


def test_far_list_full(rb, oracle16, monkeypatch):
    """TILE_WHY_FAR: 1,225 bodies leave their tile's ring in one step.  They
    keep their velocity, so the tile run after the back-off fails for the
    same reason and is replayed too."""
    sc = tf.far_flood()
    assert sc.n > tf.FARMAX
    osc = oracle16.OracleScene(sc)
    q, v = oracle16.step(osc, sc.qpos0, sc.qvel0, 3)
    with _world(rb, monkeypatch, sc, cols=4) as w:
        w.step(3)
        st = w.stats()
        _after_failure(oracle16, osc, w, q, v, st, tf.WHY["FAR"], again=True)


def test_too_many_partners(rb, oracle16, monkeypatch):
    """TILE_WHY_PARTNERS: sheet_radius (24 satellites touch each r = 1 sphere)
    in a world of max_partners 16.  The replay grows max_partners as the
    synchronous rb_step of a hashed world does (a guarded run of at least 64
    steps: to 32), and the state and the records are those of the oracle at
    that capacity; later runs commit in the 32-partner kernel."""
    pb = cg.make("sheet_radius")
    sc = pb.scene(0)
    fit = tf.fit(pb.qpos, cg.column_size(pb), force=4)
    assert tf.holds(fit)
    with _world(rb, monkeypatch, sc, tile=0, max_partners=16) as h:
        h.step(64)
        grown = h.stats()["max_partners"]
        hq, hv = h.get_state()
    assert grown == 32
    osc = oracle16.OracleScene(sc, max_partners=grown)
    q, v = oracle16.step(osc, sc.qpos0, sc.qvel0, 64)
    assert _same(hq, q) and _same(hv, v)
    with _world(rb, monkeypatch, sc, cols=4, max_partners=16) as w:
        w.step(64)
        st = w.stats()
        assert st["tile_why"] == tf.WHY["PARTNERS"] and st["max_partners"] == grown, (st, grown)
        _grid_is(st, fit)
        _after_failure(oracle16, osc, w, q, v, st, tf.WHY["PARTNERS"])
        assert w.stats()["max_partners"] == grown


def test_auto_mode_after_a_failure_steps_hashed(rb, oracle16, monkeypatch):
    """The far-list failure in auto mode (RBHIP_TILE_MIN_BODIES lowered so the
    scene qualifies): the roll-back retires the tile form, further runs step
    hashed and follow the oracle."""
    sc = tf.far_flood()
    osc = oracle16.OracleScene(sc)
    q, v = oracle16.step(osc, sc.qpos0, sc.qvel0, 3)
    monkeypatch.setenv("RBHIP_TILE_MIN_BODIES", "1")
    fit = tf.fit(sc.qpos0, tf.COL)                      # (unforced: auto mode takes the form only where the bins stay small)
    assert tf.holds(fit) and fit.slots <= sc.n // 20, fit
    with _world(rb, monkeypatch, sc, tile=None) as w:
        monkeypatch.delenv("RBHIP_TILE_MIN_BODIES")
        w.step(3)
        st = w.stats()
        _grid_is(st, fit)
        assert st["tile_rollbacks"] == 1 and st["tile_why"] & tf.WHY["FAR"] and st["tile_steps"] == 0, st
        _state_is(w, q, v, "after the replay")
        for k in range(2):
            q, v = oracle16.step(osc, q, v, 2)
            w.step(2)
            _state_is(w, q, v, f"after further run {k}")
        st = w.stats()
    assert st["form"] != tf.FORM_TILE and st["tile_on"] == 0 and st["tile_rollbacks"] == 1 and st["tile_steps"] == 0, st


def test_out_of_domain(rb, monkeypatch):
    """TILE_WHY_DOMAIN: one sphere's velocity takes it past 2^29 columns in
    the first step.  The tile run raises the reason and is replayed; the
    replay ends as the same scene does with the tile form off: the same
    RbError code, the two worlds in the same state."""
    sc = tf.domain_runaway()
    left = {}
    for tile in (0, 1):
        with _world(rb, monkeypatch, sc, tile=tile) as w:
            with pytest.raises(rb.RbError) as e:
                w.step(2)
            left[tile] = (e.value.code, w.stats(), w.get_state())
    (c0, s0, (q0, v0)), (c1, s1, (q1, v1)) = left[0], left[1]
    assert c0 == c1 == EDOM, (c0, c1)
    assert s0["tile_runs"] == 0 and s1["tile_runs"] == 1 and s1["tile_why"] & tf.WHY["DOMAIN"] \
        and s1["tile_rollbacks"] == 1 and s1["tile_steps"] == 0, (s0, s1)
    assert _same(q0, q1) and _same(v0, v1)
