"""tests/tile_fit.py on the CPU: the mirror of the tile fit on inputs whose
answer follows by hand, and the preconditions of every case of
tests/test_gpu_tile_edges.py: from the mirror and the oracle's trajectory,
each scene reaches the path it is meant to reach before a GPU sees it (the
tile-shaped families of contact_geometry have theirs in
tests/test_oracle_contact_geometry.py sheet_claims)."""
import numpy as np
import pytest

import tile_fit as tf

COL = tf.COL


def _centres(cols):
    """One body in the middle of each listed column (repeats: several)."""
    return (np.asarray(cols, float) + 0.5) * COL


def _block(nx, ny, per=1, x0=0, y0=0):
    return _centres([(x0 + x, y0 + y) for y in range(ny) for x in range(nx) for _ in range(per)])


# ------------------------------------------------------------ the mirror
def test_constants_agree_with_contact_geometry():
    import contact_geometry as cg
    assert tf.COL == cg.COARSE and tf.R0 == cg.R0 and tuple(range(tf.TC_MIN, tf.TC_MAX + 1)) == cg.SHEET_TC


def test_width_from_density():
    # 80 / per-column -> 1: sqrt 80 = 8.9 -> clamped 8; 3: 5.16 -> 5; 5: 4; 40: 1.4 -> clamped 4
    for per, tc in ((1, 8), (3, 5), (5, 4), (40, 4)):
        f = tf.fit(_block(16, 16, per), COL)
        assert f.tc_free == tc, (per, f)
    # half-way cases round away from zero like lround: 80 / 12.8 = 6.25 -> 2.5 -> 3 -> clamped 4
    assert tf.fit(_block(5, 1, 64), COL).tc == 4


def test_width_lowered_under_the_112_rule():
    # 2 per column: a tile of width 8 holds 128 > 112, of width 7 at most 98
    f = tf.fit(_block(32, 32, 2), COL, force=8)
    assert (f.tc_free, f.tc, f.worst_tile) == (8, 7, 98)
    # 3 per column: 8 -> 192, 7 -> 147, 6 -> 108
    f = tf.fit(_block(24, 24, 3), COL, force=8)
    assert (f.tc, f.worst_tile) == (6, 108)
    # never below 4, whatever the tile holds; a forced width is clamped to 4 .. 8
    f = tf.fit(_block(8, 8, 10), COL, force=5)
    assert (f.tc, f.worst_tile) == (4, 160) and not tf.holds(f)
    assert tf.fit(_block(8, 8), COL, force=2).tc == 4 and tf.fit(_block(8, 8), COL, force=11).tc == 8


def test_grid_extent_and_negative_columns():
    # columns -5 .. 10 in x (15 // 4 + 3 = 6 tiles), -1 .. 0 in y (0 + 3)
    xy = _centres([(-5, -1), (10, 0), (0, 0)])
    f = tf.fit(xy, COL, force=4)
    assert (f.ntx, f.nty, f.slots, f.folded) == (6, 3, 18, False)
    assert sorted(map(tuple, f.tiles.tolist())) == [(-2, -1), (0, 0), (2, 0)]
    # a coordinate just below 0 lies in column -1, tile -1
    f = tf.fit(np.array([[-1e-9, -1e-9], [1e-9, 1e-9]]), COL)
    assert sorted(map(tuple, f.tiles.tolist())) == [(-1, -1), (0, 0)]
    # non-finite and far-out positions take no part, the body count still sets the slots' cap
    f = tf.fit(np.array([[0.1, 0.1], [np.nan, 0.0], [1e12, 0.0], [0.0, np.inf]]), COL)
    assert (f.ntx, f.nty, int(f.slot_n.sum())) == (3, 3, 1)


def test_fold():
    # 48 bodies: max_slots = 4 * 2 + 64 = 72.  Columns 0 .. 399 in x: 399 // 4 + 3 = 102 tiles by 3:
    # 306 -> 51 x 3 = 153 -> 26 x 3 = 78 -> 13 x 3 = 39
    cols = [(int(x), 0) for x in np.linspace(0, 399, 48).round()]
    f = tf.fit(_centres(cols), COL, force=4)
    assert (f.ntx, f.nty, f.folded) == (13, 3, True)
    # the period is 52 columns: columns 0 and 52 share a column of the folded grid, tiles 0 and 13 a slot
    g = tf.fit(_centres([(0, 0), (52, 0)] + cols), COL, force=4, n=48)
    assert (g.ntx, g.nty) == (13, 3) and g.cols[0, 0] == 3 and g.aliased >= 2
    # exactly max_slots is not folded
    f = tf.fit(_centres([(0, 0), (4 * 21 - 1, 0)] * 24), COL, force=4)
    assert (f.ntx, f.nty, f.folded) == (23, 3, False) and 4 * 2 + 64 >= 69


def test_windows_and_columns():
    # tile (0, 0) of width 4 empty but for one body; 5 bodies in each column that touches it from outside
    ring = [(x, y) for x in range(-1, 5) for y in range(-1, 5) if x in (-1, 4) or y in (-1, 4)]
    xy = np.concatenate([_centres([c for c in ring for _ in range(5)]), _centres([(2, 1)])])
    f = tf.fit(xy, COL, force=4)
    sx, sy = 0 % f.ntx, 0 % f.nty
    assert f.slot_n[sy, sx] == 1 and f.window[sy, sx] == 5 * 20 + 1
    wc = f.window_cols[sy, sx]
    assert wc[1 + 1, 2 + 1] == 1 and (wc[0, :] == 5).all() and (wc[:, -1] == 5).all() and wc[1:-1, 1:-1].sum() == 1
    # the tile to the west holds the ring's west side, rows 0 .. 3, in its column 3
    west = f.window_cols[sy, (sx - 1) % f.ntx]
    assert (west[1:5, 4] == 5).all() and f.slot_n[sy, (sx - 1) % f.ntx] == 20
    assert f.worst_column == 5 and not (f.cols > tf.WR).any()
    # a later state under the same grid: everything one column to the east (the west side's rows 0 .. 3 move in)
    g = tf.refit(f, xy + [COL, 0.0], COL)
    assert (g.tc, g.ntx, g.nty) == (f.tc, f.ntx, f.nty) and g.slot_n[sy, sx] == 1 + 4 * 5


# ------------------------------------------------------------ the GPU cases' preconditions
@pytest.fixture(scope="module")
def orc(oracle):
    oracle.set_threads(8)
    yield oracle
    oracle.set_threads(1)


def _trajectory(oracle, sc, steps, **kw):
    osc = oracle.OracleScene(sc, **kw)
    q, v, out = sc.qpos0, sc.qvel0, [sc.qpos0]
    for _ in range(steps):
        q, v = oracle.step(osc, q, v, 1)
        out.append(q)
    return out


def _holds_along(f, qs):
    later = [tf.refit(f, q, COL) for q in qs]
    return max(x.worst_slot for x in later) <= tf.FIT_MAX and max(x.worst_window for x in later) <= tf.WMAX


def test_falling_grid_holds_every_width_and_crosses_tiles(orc):
    sc = tf.falling_grid()
    assert 2200 <= sc.n <= 2400
    qs = _trajectory(orc, sc, 63)
    assert tf.fit(sc.qpos0, COL).tc == 8
    for tc in range(4, 9):
        f = tf.fit(sc.qpos0, COL, force=tc)
        assert f.tc == tc and not f.folded and f.slots <= tf.OCC3_SLOTS and _holds_along(f, qs), f
        t0, t1 = (np.floor_divide(tf.columns(q, COL), tc) for q in (qs[0], qs[60]))
        for a in range(2):
            assert ((t1 - t0)[:, a] > 0).sum() >= 20 and ((t1 - t0)[:, a] < 0).sum() >= 20, (tc, a)


@pytest.mark.parametrize("tile0", [(2, 2), (-9, -8)])
def test_ring_movers_cover_every_displacement(orc, tile0):
    sc, start, disp, ids = tf.ring_movers(tc=4, tile0=tile0)
    f = tf.fit(sc.qpos0, COL, force=4)
    qs = _trajectory(orc, sc, 5)
    assert f.tc == 4 and not f.folded and _holds_along(f, qs), f
    c0, c1 = tf.columns(qs[0], COL)[ids], tf.columns(qs[1], COL)[ids]
    t0 = np.floor_divide(c0, 4)
    assert ((t0 < 0).all() if tile0[0] < 0 else (t0 > 0).all())
    at = c0 - 4 * t0                                     # the start column within the tile
    moved = c1 - c0
    assert (at == start).all() and (moved == disp).all()
    assert set(map(tuple, moved.tolist())) == set(tf.DISPLACEMENTS) and len(tf.DISPLACEMENTS) == 25
    # the tile is interior: populated or not, every neighbour is a slot of its own
    assert f.ntx >= 9 and f.nty >= 9
    new = at + moved                                     # the column after the step, relative to the start tile
    ring = ((new >= -1) & (new <= 4)).all(1) & ((new < 0) | (new > 3)).any(1)
    far = ((new < -1) | (new > 4)).any(1)
    places = {"w": new[:, 0] == -1, "e": new[:, 0] == 4, "s": new[:, 1] == -1, "n": new[:, 1] == 4}
    one = np.abs(moved).max(1) == 1
    for side, m in places.items():                       # out by one column over each edge ...
        along = new[:, 1 if side in "we" else 0]
        assert (ring & one & m & (along >= 0) & (along <= 3)).any(), side
    for a, b in (("w", "s"), ("w", "n"), ("e", "s"), ("e", "n")):    # ... and over each corner
        assert (ring & one & places[a] & places[b]).any(), (a, b)
    assert far.sum() >= 40 and ring.sum() >= 40
    # every mover overlaps its target after the first step and not before (but the one that stays)
    d0 = np.linalg.norm(qs[0][ids, :3] - qs[0][ids + 1, :3], axis=1)
    d1 = np.linalg.norm(qs[1][ids, :3] - qs[1][ids + 1, :3], axis=1)
    still = (disp == 0).all(1)
    assert (d1 < 0.19).all() and (d0[~still] > 0.21).all()
    # four far arrivals in a ring column of their target's window, one per side (east: column tc, the
    # far list's admission bound), overlapping the target only after the step
    m, t, at = tf.ring_arrivals(sc)
    assert sorted(map(tuple, at.tolist())) == [(-1, 1), (1, -1), (1, 4), (4, 1)]
    assert (np.abs(tf.columns(qs[1], COL)[m] - tf.columns(qs[0], COL)[m]).max(1) == 4 + 2).all()
    assert (np.linalg.norm(qs[1][m, :3] - qs[1][t, :3], axis=1) < 0.16).all()
    assert (np.linalg.norm(qs[0][m, :3] - qs[0][t, :3], axis=1) > 2.0).all()
    # the second step's records: every target lists its mover and nothing else, every mover its target
    osc = orc.OracleScene(sc)
    cnt, par = orc.step(osc, qs[1], np.zeros((sc.n, 6)), 1, record=True)[2][:2]    # (records: of the positions alone)
    first = np.concatenate([[0], np.cumsum(cnt)])
    pairs = np.concatenate([np.stack([ids, ids + 1], 1), np.stack([m, t], 1)])
    assert (cnt[pairs] == 1).all() and cnt.sum() == 2 * len(pairs)
    assert (par[first[pairs[:, 0]]] == pairs[:, 1]).all() and (par[first[pairs[:, 1]]] == pairs[:, 0]).all()
    # no window holds more far bodies than it may
    near = np.abs(c1[far][:, None, :] - c1[far][None, :, :]).max(2) <= 4 + 2         # (a window is 6 columns wide)
    assert near.sum(1).max() <= tf.FARWIN and far.sum() <= tf.FARMAX


def test_far_movers_leave_their_rings(orc):
    sc, who = tf.far_movers()
    assert sc.n == 1024
    f = tf.fit(sc.qpos0, COL)
    qs = _trajectory(orc, sc, 40)
    assert _holds_along(f, qs), f
    moved = np.abs(tf.columns(qs[1], COL)[who] - tf.columns(qs[0], COL)[who]).max(1)
    assert (moved >= 2).sum() >= 4 and moved.max() > f.tc + 1


def test_fold_patches_alias(orc):
    sc = tf.fold_patches()
    f = tf.fit(sc.qpos0, COL, force=4)
    assert 1900 <= sc.n <= 2100 and f.tc == 4 and f.folded and f.aliased >= 24, f
    assert _holds_along(f, _trajectory(orc, sc, 63))
    # both patches on shared slots: a slot holds more than any one tile
    assert f.worst_slot > f.worst_tile


def test_sparse_grid_takes_the_three_wave_kernel(orc):
    sc = tf.sparse_grid()
    f = tf.fit(sc.qpos0, COL, force=4)
    assert 7500 <= sc.n <= 10000 and f.tc == 4 and f.slots > tf.OCC3_SLOTS and not f.folded, f
    assert _holds_along(f, _trajectory(orc, sc, 43))
    assert tf.fit(tf.falling_grid().qpos0, COL, force=4).slots <= tf.OCC3_SLOTS      # (the other sizing)


def test_falling_piles_reach_the_pile_path(orc):
    sc, sl = tf.falling_piles()
    f = tf.fit(sc.qpos0, COL)
    assert sc.n <= 3000 and f.tc == 4 and not f.folded and tf.holds(f), f
    ring = f.window_cols.copy()
    ring[:, :, 1:-1, 1:-1] = 0
    assert (f.cols > tf.WR).sum() >= 50 and f.worst_column > 12 and ring.max() > 12, f
    qs = _trajectory(orc, sc, 43)
    for q in qs:                                          # no slot past 128, no window past 384: no roll-back is due
        later = tf.refit(f, q, COL)
        assert later.worst_slot <= tf.THREADS and later.worst_window <= tf.WMAX, later
    rest = np.setdiff1d(np.arange(sc.n), sl)
    assert min(q[sl, 2].min() - q[rest, 2].max() for q in qs) > 0.5       # the sliders pass over the stacks
    # after the first step every body is in the bin of the tile it started in (none moved two columns).
    # A slider then stands one column outside its tile, in that bin's ring, over a stack of the
    # neighbour's own bin: a window column of more than WR records whose records past the first WR
    # run from one source bin into the second
    c0, c1 = tf.columns(qs[0], COL), tf.columns(qs[1], COL)
    assert np.abs(c1 - c0).max() == 1
    bin0 = np.floor_divide(c0, 4)
    fed = 0
    for col in np.unique(c1[sl], axis=0):
        here = (c1 == col).all(1)
        own = here & (bin0 == np.floor_divide(col, 4)).all(1)
        fed += int(0 < own.sum() < here.sum() and here.sum() > tf.WR and (here & ~own)[sl].sum() == 8)
    assert fed == 3


def test_failure_scenes_fail_for_their_reason(orc):
    # WINDOW by records: every tile within the fit's limit at width 8, one window past 384
    sc = tf.window_stacks()
    f = tf.fit(sc.qpos0, COL, force=8)
    assert sc.n <= 3000 and f.tc == 8 and f.worst_slot <= tf.FIT_MAX and f.worst_window > tf.WMAX, f
    assert int((f.window > tf.WMAX).sum()) == 1
    free = tf.fit(sc.qpos0, COL)
    assert free.tc == 4 and tf.holds(free), free
    # WINDOW by far bodies: all movers far after every step, apart until step 4, over one column then
    sc = tf.far_throw()
    f = tf.fit(sc.qpos0, COL, force=4)
    qs = _trajectory(orc, sc, 8)
    mv = np.arange(sc.n - 40, sc.n)
    cs = [tf.columns(q, COL) for q in qs]
    for k in range(1, 6):
        assert (cs[k][mv, 0] - cs[k - 1][mv, 0] >= 2 * 4).all()          # past the ring from any start column
    for k in range(0, 4):
        win = np.floor_divide(np.mod(cs[k][mv], [f.ntx * 4, f.nty * 4]), 4)
        assert np.unique(win, axis=0, return_counts=True)[1].max() <= tf.FARWIN // 3, k
    assert len(np.unique(cs[4][mv], axis=0)) == 1 and len(mv) > tf.FARWIN
    assert _holds_along(f, qs[:4]) and max(tf.refit(f, q, COL).worst_slot for q in qs) <= tf.THREADS
    # FAR: more than 1,024 bodies past the ring in one step
    sc = tf.far_flood()
    q1 = _trajectory(orc, sc, 1)[1]
    assert sc.n <= 3000 and ((tf.columns(q1, COL) - tf.columns(sc.qpos0, COL))[:, 0] >= 8).sum() > tf.FARMAX
    assert tf.holds(tf.fit(sc.qpos0, COL, force=4))
    # DOMAIN: one body past 2^29 columns after a finite step
    sc = tf.domain_runaway()
    x1 = sc.qpos0[:, 0] + sc.dt * sc.qvel0[:, 0]
    assert np.isfinite(x1).all() and (np.abs(x1 / COL) >= 2.0 ** 29).sum() == 1
    assert tf.holds(tf.fit(sc.qpos0, COL))
