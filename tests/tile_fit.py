"""A plain NumPy mirror of the tile form's fit (csrc/rb_api_tiles.hip
tile_fit), and the scenes of tests/test_gpu_tile_edges.py.

fit(xy, col, force=None) restates tile_fit from positions and the column
size (the hashed cell, 4 rmax 1.001): the tile width tc (the rounded
sqrt(80 / bodies per occupied column), clamped to 4 .. 8, or the forced
RBHIP_TILE_COLS; lowered while the densest tile holds more than 7/8 x 128
bodies), and the slot grid ntx x nty after the fold under
max_slots = 4 ceil(N / 24) + 64.  On top of what the library computes it
counts what the step kernel will meet: per tile and per slot (the tiles a
fold puts on one slot add up) the bodies, per window (a slot's columns plus
its ring of one column) the records, and per window column its records.  A
window column's count does not depend on which bin holds a body (its own
tile's, or a neighbour's ring), so the counts hold for any state whose
bodies are all binned; bodies on the far list are not window records.

The tests use it twice: on the CPU, to show that a scene reaches the path
it is meant to reach (the densest tile at most 112, the largest window at
most 384 where a run must commit and more where it must not, the fold
taken or not); on the GPU, where stats()["tile_cols"] and ["tile_slots"]
must equal the mirror's.
"""
import math

import numpy as np

THREADS = 128            # TILE_THREADS: a slot steps at most this many bodies
FIT_MAX = 7 * THREADS // 8
WMAX = 384               # TILE_WMAX: window records
FARWIN = 32              # TILE_FARWIN: far bodies one window holds
FARMAX = 1024            # TILE_FARMAX
WR = 6                   # records per window column staged in registers (more: the pile path)
OCC3_SLOTS = 1024        # TILE_OCC3_SLOTS
TC_MIN, TC_MAX = 4, 8
WHY = {"CAP": 1, "WINDOW": 2, "FAR": 4, "PARTNERS": 8, "DOMAIN": 16}
FORM_TILE = 5

R0 = 0.1
COL = 4 * R0 * 1.001     # the column of a world of r = 0.1 spheres


class Fit:
    """tc, ntx, nty, slots; tc_free (before the 112 rule); folded; tiles: the
    populated tiles (T, 2) and their counts tile_n; slot_n (nty, ntx): bodies
    per slot; cols (nty tc, ntx tc): records per column of the folded grid;
    window (nty, ntx): records per window; window_cols (nty, ntx, tc + 2,
    tc + 2): records per window column; aliased: populated tiles on a slot
    that another populated tile shares."""

    @property
    def worst_tile(self):
        return int(self.tile_n.max()) if self.tile_n.size else 0

    @property
    def worst_slot(self):
        return int(self.slot_n.max())

    @property
    def worst_window(self):
        return int(self.window.max())

    @property
    def worst_column(self):
        return int(self.cols.max())

    def __repr__(self):
        return (f"Fit(tc={self.tc}, {self.ntx}x{self.nty}, folded={self.folded}, tile<={self.worst_tile}, "
                f"slot<={self.worst_slot}, window<={self.worst_window}, column<={self.worst_column}, aliased={self.aliased})")


def columns(xy, col):
    """Integer columns of positions, as tile_fit takes them: floor(x * (1 / col))."""
    inv = 1.0 / col
    f = np.asarray(xy, np.float64)[:, :2] * inv
    ok = (np.abs(f[:, 0]) < 1e9) & (np.abs(f[:, 1]) < 1e9)
    return np.floor(f[ok]).astype(np.int64)


def _worst_tile(c, tc):
    if not len(c):
        return 0
    return int(np.unique(np.floor_divide(c, tc), axis=0, return_counts=True)[1].max())


def fit(xy, col, force=None, n=None):
    """The mirror.  xy (N, 2+): positions; col: the column size; force: the
    value of RBHIP_TILE_COLS; n: the world's body count (default len(xy))."""
    c = columns(xy, col)
    n = len(xy) if n is None else n
    f = Fit()
    if len(c):
        lo, hi = c.min(0), c.max(0)
    else:
        lo, hi = np.zeros(2, np.int64), np.zeros(2, np.int64)
    nocc = max(1, len(np.unique(c, axis=0))) if len(c) else 1
    per_col = max(1, len(c)) / nocc
    tc = int(math.floor(math.sqrt(80.0 / per_col) + 0.5))
    tc = max(TC_MIN, min(TC_MAX, tc))
    if force is not None:
        tc = max(TC_MIN, min(TC_MAX, int(force)))
    f.tc_free = tc
    while tc > TC_MIN and _worst_tile(c, tc) > FIT_MAX:
        tc -= 1
    # (C division of non-negative extents)
    ntx, nty = int(hi[0] - lo[0]) // tc + 3, int(hi[1] - lo[1]) // tc + 3
    max_slots = 4 * ((n + 23) // 24) + 64
    f.folded = ntx * nty > max_slots
    while ntx * nty > max_slots:
        if ntx >= nty:
            ntx = (ntx + 1) // 2
        else:
            nty = (nty + 1) // 2
    f.tc, f.ntx, f.nty = tc, max(3, ntx), max(3, nty)
    f.slots = f.ntx * f.nty
    count(f, c)
    return f


def count(f, c):
    """What the kernel meets under the grid of f for bodies in columns c."""
    tc, ntx, nty = f.tc, f.ntx, f.nty
    t = np.floor_divide(c, tc)
    f.tiles, f.tile_n = np.unique(t, axis=0, return_counts=True) if len(c) else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    f.slot_n = np.zeros((nty, ntx), np.int64)
    np.add.at(f.slot_n, (np.mod(t[:, 1], nty), np.mod(t[:, 0], ntx)), 1)
    shared = np.zeros((nty, ntx), np.int64)
    np.add.at(shared, (np.mod(f.tiles[:, 1], nty), np.mod(f.tiles[:, 0], ntx)), 1)
    f.aliased = int(shared[shared > 1].sum())
    Px, Py = ntx * tc, nty * tc
    f.cols = np.zeros((Py, Px), np.int64)
    np.add.at(f.cols, (np.mod(c[:, 1], Py), np.mod(c[:, 0], Px)), 1)
    f.window_cols = np.zeros((nty, ntx, tc + 2, tc + 2), np.int64)
    for vy in range(-1, tc + 1):
        for vx in range(-1, tc + 1):
            f.window_cols[:, :, vy + 1, vx + 1] = np.roll(f.cols, (-vy, -vx), (0, 1))[::tc, ::tc]
    f.window = f.window_cols.sum((2, 3))
    return f


def refit(f, xy, col):
    """The counts of a later state under the grid fitted earlier (a run keeps
    its grid while the bodies move)."""
    g = Fit()
    g.tc, g.ntx, g.nty, g.slots, g.tc_free, g.folded = f.tc, f.ntx, f.nty, f.slots, f.tc_free, f.folded
    return count(g, columns(xy, col))


def holds(f):
    """A run on this state can commit: no slot past the fit's 112, no window past 384."""
    return f.worst_slot <= FIT_MAX and f.worst_window <= WMAX


# ---------------------------------------------------------------- scenes
def _scene(name, c, v=None, gravity=(0.0, 0.0, 0.0), floor=-50.0, r=R0, restitution=0.5, friction=0.4):
    """Spheres of radius r (unit mass and inertia) at centres c with linear
    velocities v over a floor z = floor."""
    from rbhip import scenes
    c = np.asarray(c, float)
    n = len(c)
    q = np.zeros((n, 7))
    q[:, :3], q[:, 3] = c, 1.0
    qv = np.zeros((n, 6))
    if v is not None:
        qv[:, :3] = v
    size = np.zeros((n, 3))
    size[:, 0] = r
    return scenes.Scene(name, np.zeros(n, np.int32), np.ones(n), np.ones((n, 3)), size,
                        np.array([[0.0, 0, 1, 0, 0, floor]]), q, qv, dt=0.01, restitution=restitution,
                        friction=friction, threshold=0.0, gravity=np.asarray(gravity, float))


def grid(nx, ny, seed, spacing=0.3, vxy=0.3, at=(0.0, 0.0)):
    """scenes.flat_spheres with a horizontal velocity spread of vxy, centred at `at`."""
    from rbhip import scenes
    sc = scenes.flat_spheres(nx, ny, seed=seed, spacing=spacing)
    q, v = sc.qpos0.copy(), sc.qvel0.copy()
    q[:, 0] += at[0]
    q[:, 1] += at[1]
    v[:, 0:2] *= vxy / 0.3
    return sc.with_(qpos0=q, qvel0=v)


def join(a, b):
    """Two sphere scenes of the same parameters as one."""
    cat = lambda k: np.concatenate([getattr(a, k), getattr(b, k)])      # noqa: E731
    return a.with_(name=a.name + "+" + b.name, kind=cat("kind"), mass=cat("mass"), inertia=cat("inertia"),
                   size=cat("size"), qpos0=cat("qpos0"), qvel0=cat("qvel0"))


DISPLACEMENTS = [(ex, ey) for ey in range(-2, 3) for ex in range(-2, 3)]
# start columns inside a tile of width tc: the four corners, the four edges' middles
def ring_starts(tc):
    m = tc // 2
    return {"sw": (0, 0), "se": (tc - 1, 0), "nw": (0, tc - 1), "ne": (tc - 1, tc - 1),
            "w": (0, m), "e": (tc - 1, m), "s": (m, 0), "n": (m, tc - 1)}


def ring_movers(tc=4, tile0=(2, 2), seed=0, dt=0.01):
    """Movers for the ring and the far list.  Eight tiles of width tc, three
    tiles apart from (tile0) on (3 x 3 spots without the middle one, which
    holds four far arrivals: below), one per start column of ring_starts(); in
    each, 25 movers stacked 0.25 apart in z over that column, one per
    displacement (ex, ey) in {-2 .. 2}^2 columns per step, each with a resting
    target at its own height which it overlaps (centre distance 0.15) where
    it arrives after one step.  No gravity: every body keeps its height.
    Returns (scene, start (200, 2) the movers' start columns within their
    tile, disp (200, 2), mover ids)."""
    rng = np.random.default_rng(seed)
    c, v, start, disp = [], [], [], []
    for k, (name, (sx, sy)) in enumerate(ring_starts(tc).items()):
        spot = k if k < 4 else k + 1                     # (the middle of the 3 x 3 spots: the far arrivals below)
        tx, ty = tile0[0] + 3 * (spot % 3), tile0[1] + 3 * (spot // 3)
        for layer, (ex, ey) in enumerate(DISPLACEMENTS):
            frac = rng.uniform(0.3, 0.7, 2)
            p = np.array([(tx * tc + sx + frac[0]) * COL, (ty * tc + sy + frac[1]) * COL, 1.0 + 0.25 * layer])
            d = np.array([ex * COL, ey * COL, 0.0])
            a = rng.uniform(0, 2 * np.pi)
            c.append(p)
            v.append(d / dt)
            c.append(p + d + 0.15 * np.array([np.cos(a), np.sin(a), 0.0]))
            v.append(np.zeros(3))
            start.append((sx, sy))
            disp.append((ex, ey))
    ids = np.arange(0, len(c), 2)
    # far arrivals just across a tile boundary from their target: in the middle
    # tile four targets 0.2 columns inside its east, west, north and south
    # edge, each at its own height, and for each a mover that starts tc + 2
    # columns further out (so it goes to the far list) and lands 0.15 beyond
    # the target, in the ring column of the target's window
    tx, ty = tile0[0] + 3, tile0[1] + 3
    for layer, (ax, sign) in enumerate(((0, 1), (0, -1), (1, 1), (1, -1))):
        t = np.array([(tx * tc + 1.5) * COL, (ty * tc + 1.5) * COL, 1.0 + 0.25 * (len(DISPLACEMENTS) + layer)])   # (above the rest)
        t[ax] = ((tx, ty)[ax] * tc + (tc - 0.2 if sign > 0 else 0.2)) * COL
        d = np.zeros(3)
        d[ax] = -sign * (tc + 2) * COL
        land = t.copy()
        land[ax] += sign * 0.15
        c += [land - d, t]
        v += [d / dt, np.zeros(3)]
    sc = _scene("ring_movers", c, v)
    return sc, np.array(start), np.array(disp), ids


def ring_arrivals(sc, tc=4):
    """ring_movers' last eight bodies: (mover ids, target ids, the column
    (vx, vy) of each mover after one step within its target's window)."""
    m, t = np.arange(sc.n - 8, sc.n, 2), np.arange(sc.n - 7, sc.n, 2)
    land = sc.qpos0[m, :2] + sc.dt * sc.qvel0[m, :2]
    return m, t, columns(land, COL) - tc * np.floor_divide(columns(sc.qpos0[t], COL), tc)


def piles(tiles=5, tc=4, seed=0, tile0=(-3, -3), gap=1e-3):
    """Vertical stacks of 7 to 20 spheres, neighbours 2 r (1 - gap) apart, the
    lowest resting gap r deep in the floor z = 0; three to five stacks per
    tile of width tc on tiles x tiles tiles from tile0 on, in columns drawn
    with the tile's edge columns first, and in every third tile two stacks in
    one column (at a quarter and at three quarters of its diagonal).  Returns
    (centres, expect: the records each body has at rest)."""
    rng = np.random.default_rng(seed)
    c, expect = [], []
    step = 2 * R0 * (1 - gap)
    for t in range(tiles * tiles):
        tx, ty = tile0[0] + t % tiles, tile0[1] + t // tiles
        edge = [(x, y) for x in range(tc) for y in range(tc) if x in (0, tc - 1) or y in (0, tc - 1)]
        cols = [edge[i] for i in rng.permutation(len(edge))[:rng.integers(3, 6)]]
        spots = [(cx, cy, 0.25) for cx, cy in cols]
        if t % 3 == 0:
            spots.append((cols[0][0], cols[0][1], 0.75))
        for cx, cy, fr in spots:
            h = int(rng.integers(7, 21))
            x, y = (tx * tc + cx + fr) * COL, (ty * tc + cy + fr) * COL
            for k in range(h):
                c.append([x, y, R0 * (1 - gap) + k * step])
                expect.append((2 if 0 < k < h - 1 else 1) + (1 if k == 0 else 0))
    return np.array(c), np.array(expect)


def window_stacks(tc=8, h=13):
    """TILE_WHY_WINDOW by records: the four rows of columns that touch the
    tile (0, 0) of width tc from outside hold a stack of h spheres per column
    (tc h bodies in each neighbour tile), the tile itself four spheres."""
    c = []
    step = 2 * R0 * (1 - 1e-3)
    for k in range(tc):
        for cx, cy in ((k, tc), (k, -1), (tc, k), (-1, k)):
            for z in range(h):
                c.append([(cx + 0.5) * COL, (cy + 0.5) * COL, R0 * (1 - 1e-3) + z * step])
    for cx, cy in ((1, 1), (tc - 2, 2), (3, tc - 2), (tc // 2, tc // 2)):
        c.append([(cx + 0.5) * COL, (cy + 0.5) * COL, 0.5])
    return _scene("window_stacks", c, gravity=(0, 0, -9.81), floor=0.0)


def far_throw(n_movers=40, arrive=4, tc=4, seed=0, dt=0.01):
    """TILE_WHY_WINDOW by far bodies: a 16 x 16 patch about the origin, and
    n_movers spheres on the line y = 0.5 columns, 0.25 apart in z, mover i
    moving 2 tc + i columns a step in x (so it is on the far list after
    every step) from arrive x (2 tc + i) columns before column 1: after
    `arrive` steps all stand over column 1, and the step after finds more
    than 32 far bodies in one window.  Before that no two movers share a
    column."""
    sc = grid(16, 16, seed, vxy=1.0)
    sc = sc.with_(gravity=np.zeros(3), planes=np.array([[0.0, 0, 1, 0, 0, -50.0]]))
    i = np.arange(n_movers)
    per = 2 * tc + i
    c = np.stack([(1.5 - arrive * per) * COL, np.full(n_movers, 0.5 * COL), 3.0 + 0.25 * i], 1)
    v = np.stack([per * COL / dt, np.zeros(n_movers), np.zeros(n_movers)], 1)
    mv = _scene("movers", c, v)
    mv = mv.with_(mass=np.full(n_movers, sc.mass[0]), inertia=np.tile(sc.inertia[0], (n_movers, 1)),
                  restitution=sc.restitution, friction=sc.friction)
    return join(sc, mv)


def far_flood(nx=35, ny=35, tc=8, dt=0.01):
    """TILE_WHY_FAR: nx ny resting spheres 0.3 apart, all moving 2 tc + 0.3
    columns a step in x: every one leaves its tile's ring in the first step,
    whatever the width up to tc."""
    sc = grid(nx, ny, 1, vxy=0.0)
    v = sc.qvel0.copy()
    v[:, 0] = (2 * tc + 0.3) * COL / dt
    return sc.with_(qvel0=v, gravity=np.zeros(3), planes=np.array([[0.0, 0, 1, 0, 0, -50.0]]))


def domain_runaway(dt=0.01):
    """TILE_WHY_DOMAIN: a 12 x 12 patch, and one sphere whose velocity takes it
    past 2^29 columns in the first step."""
    sc = grid(12, 12, 2)
    v = sc.qvel0.copy()
    v[5, 0] = 1.5 * 2.0 ** 29 * COL / dt
    return sc.with_(qvel0=v)


def falling_grid():
    """About 2,300 falling, colliding spheres 0.36 apart (at width 8 a tile
    holds about 80), horizontal velocities of 1 m/s spread."""
    return grid(48, 48, 11, spacing=0.36, vxy=1.0)


def far_movers(nx=32, ny=32, fast=6):
    """test_gpu_tiles.py's far movers at a quarter of the size: nx ny falling
    spheres, `fast` of them thrown at up to 400 m/s (10 columns a step)."""
    from rbhip import scenes
    sc = scenes.flat_spheres(nx, ny, seed=5)
    rng = np.random.default_rng(7)
    who = rng.choice(sc.n, fast, replace=False)
    v = sc.qvel0.copy()
    v[who, 0] = rng.uniform(-400.0, 400.0, fast)
    v[who, 1] = rng.uniform(-400.0, 400.0, fast)
    return sc.with_(qvel0=v), who


def fold_patches(apart=1634):
    """Two falling 32 x 32 patches `apart` columns apart in x: the grid between
    them would take more slots than the fit allows, so it folds, and tiles of
    both patches share slots."""
    return join(grid(32, 32, 8, vxy=1.0), grid(32, 32, 9, vxy=1.0, at=(apart * COL, 0.0)))


def sparse_grid():
    """About 8,000 falling spheres 0.55 apart: more than 1,024 slots at width 4."""
    return grid(90, 90, 12, spacing=0.55, vxy=1.0)


def falling_piles(seed=0, tc=4, sliders=3, dt=0.01):
    """piles() under gravity on the floor z = 0, and `sliders` groups of 8
    spheres, 0.25 apart in z from z = 6 up (above every stack for the whole
    run), that move one column a step to the west.  Each starts in column 0 of
    a tile, east of a stack in the west neighbour's last column: after the
    first step it sits in its own tile's ring bin over that stack, so the
    second step reads that window column, of more than 6 records, from two
    bins (and so does every later crossing of a tile boundary over a stack).
    Returns (scene, ids of the sliders)."""
    c, _ = piles(seed=seed, tc=tc)
    cols = columns(c, COL)
    east = np.unique(cols[np.mod(cols[:, 0], tc) == tc - 1], axis=0)[:sliders]
    assert len(east) == sliders
    extra = [[(cx + 1.5) * COL, (cy + 0.5) * COL, 6.0 + 0.25 * k] for cx, cy in east for k in range(8)]
    v = np.zeros((len(c) + len(extra), 3))
    v[len(c):, 0] = -COL / dt
    sc = _scene("piles", np.concatenate([c, extra]), v, gravity=(0, 0, -9.81), floor=0.0)
    return sc, np.arange(len(c), sc.n)
