"""A plain geometric reference for the box narrowphase, and the properties a
narrowphase result must have.  Shared by tests/test_oracle_box_geometry.py
(the CPU oracle), tests/test_gpu_box_geometry.py (the device) and, for the
random generator, tests/test_oracle_boxes.py and tests/test_gpu_boxes.py.

sphere_box / box_box (csrc/rb_boxes.hpp, oracle/rb_oracle_impl.h "box pairs")
are this project's definition, and the oracle and the kernel
were written from one description, so a geometric mistake common to both
passes every device-vs-oracle comparison.  This module is the outside anchor:
NumPy long double, working from the 8 vertices of each box and point-in-box
tests only.  It has no separating-axis projection formula (the half-extent
sum), no incident / reference face and no polygon clipper, so it shares no
structure with the code it judges.

  rotation(q)              rotation matrix of the quaternion (w, x, y, z)
  vertices(c, R, h)        the 8 corners of a box
  overlap(va, vb, axis)    min(max1 - min2, max2 - min1) of the vertex projections
  min_overlap(...)         the minimum over the 3 + 3 face normals and the
                           normalised edge crosses with |cross| > 1e-6 (that
                           cut is the definition's own)
  surface_dist(p, box)     max_i(|R^T (p - c)|_i - h_i): 0 on the surface, < 0 inside
  sphere_box_ref / sphere_sphere_ref   the two closed-form pairs

Input families (FAMILIES; each a function of (n, seed) returning rows in the
kat_narrow layout kind1, kind2, c1, q1, s1, c2, q2, s2): random, aligned,
one_axis, quarter_turns, coincident, thin, near_parallel, touching.

Properties (measure() computes the residuals, assert_properties() holds them
against the bounds; numbering as in DESIGN §2.5):
  1 finite, count <= 4                2 dist <= 0, kinds in {16, 17, 32-35, 40}
  3 face kinds 32 + t in order, an edge result has one contact
  4 contacts iff min_overlap > 0 (rows with |min_overlap| < near skipped,
    at most 1 % of a family's rows except in `touching`)
  5 |n| = 1, n points from geom1 to geom2
  6 -dist <= overlap(n), overlap(n) <= 1.05 min_overlap
  7 pos +- n dist / 2 lie one on each box (edge contacts with clamped
    closest-point parameters may miss: at most 2 % of a family's edge contacts)
  8 sphere-box and sphere-sphere rows equal the closed form
  9 `touching`: the expected manifold and depth of every row
  10 rigid-motion covariance, 11 swap symmetry (random and thin; rows whose
    count or kinds differ at most 0.5 % of the rows with contacts)

Bounds.  fp64: tol 1e-12 (inputs are O(1); the worst residual of the oracle
over all families is 3.4e-15, in the covariance of `random`), near 1e-9.

fp32: measured, not guessed.  The properties were run on the oracle's fp32
restatement (oracle.kat_narrow(..., dtype="f32"): the reference's restatement
in fp32, not the kernel) over all families at the sizes and seeds of CASES.
F32_MEASURED has the worst residual of each property over all families; the
worst of all is 2.36e-6 (property 10, pos, `random`), and the bound is 8 x
that, 1.9e-5: the factor covers inputs other than these seeds.  No row of any
family was decided differently from the long-double geometry at a
|min_overlap| above 1e-12 (the `touching` rows whose 1e-12 offsets fp32
cannot represent), and no row of a family other than `touching` lay within
1e-5 of touching, so the fp32 near is 1e-5 (a few ulp of the O(1) operands,
and well above 8 x the measured figure) and property 4 holds in fp32 for every
family: F32_NO_DECISION is empty.

In fp32 the inputs themselves are rounded, so an offset of 1e-12 is no offset
and all 16 `touching` rows return a manifold.  Property 9 therefore asserts
the count of a `touching` row in fp32 only where its separation is further
than near from 0; the depth is asserted on every contact returned.

Property 9's depth is the separation along the minimum-translation axis,
max(dz, dx) - 0.8.  That is dz - 0.8 on every row but the two with dz = 0.79
and dx = 0.8 or 0.8 - 1e-12: there the cubes also touch along x, the overlap
along x (0 or 1e-12) is the minimum, and property 6 requires that axis.

Property 11: the edge axes are tried in order and each must beat the best so
far by the bias, so two edge axes within 5 % of each other can be chosen
differently when the bodies are exchanged (1 of 418 hit box rows of `random`).
Such a row counts against the 0.5 % cap like a row whose count differs.

The tests can fail: three mutants of the oracle, built apart from the tree,
fail tests/test_oracle_box_geometry.py in fp64 (DESIGN §2.5 has the table):
  edge bias 1.05 -> 1/1.05         all 8 families: property 6 (overlap(n) up to
                                   0.048 above 1.05 min_overlap), 7 (edge
                                   contacts off the surface, far above the 2 %
                                   cap), 9, 10, 11 and "face kinds only"
  incident-face sign sg inverted   all 8 families: property 4 (136 to 402 rows
                                   overlap without contacts), 9 and the hit
                                   counts of aligned, one_axis, quarter_turns
                                   and coincident
  the -z/2 shift of pos dropped    every family but `touching` (whose corner
                                   points lie on the cubes' side faces):
                                   property 7 on face contacts (0.18 to 0.47
                                   off the surface), 11 in `random`
"""
import numpy as np

LD = np.longdouble
SPHERE, BOX = 0, 1
KINDS = (16, 17, 32, 33, 34, 35, 40)
EDGE_CUT = 1e-6                         # the definition's parallel-edge cut
EDGE_BIAS = 1.05                        # the definition's edge bias

TOL = {"f64": 1e-12, "f32": 1.9e-5}     # f32: 8 x the worst of F32_MEASURED
NEAR = {"f64": 1e-9, "f32": 1e-5}
SKIP_CAP = 0.01                         # property 4
EDGE_MISS_CAP = 0.02                    # property 7
MISMATCH_CAP = 0.005                    # properties 10, 11

# family -> (rows, seed) of the CPU tests and of the fp32 measurement
CASES = {"random": (3000, 0), "aligned": (1000, 101), "one_axis": (1000, 102), "quarter_turns": (1000, 103),
         "coincident": (1000, 104), "thin": (1000, 105), "near_parallel": (1000, 106), "touching": (16, 107)}

# Worst residual of each property on the oracle's fp32 restatement over CASES
# (capped properties after their exemptions; "decision": the largest
# |min_overlap| or |dist| of a row decided differently from the geometry).
F32_MEASURED = {"5 |n|-1": 3.48e-7, "5 n.(c2-c1)": 9.79e-13, "6 -dist<=overlap(n)": 2.56e-7,
                "6 overlap(n)<=1.05min": 2.05e-12, "7 surface (face)": 5.56e-7, "7 surface (edge)": 1.89e-7,
                "8 sb dist": 1.74e-7, "8 sb pos": 2.19e-7, "8 sb normal": 1.83e-6, "8 ss dist": 1.54e-8,
                "8 ss pos": 4.77e-9, "8 ss normal": 1.00e-7, "9 dist": 9.54e-9, "10 dist": 7.75e-7,
                "10 pos": 2.36e-6, "10 normal": 1.96e-6, "11 swap": 2.98e-8, "decision": 1.0e-12}
F32_NO_DECISION = ()                    # families whose property 4 is dropped in fp32: none

_SIGNS = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], LD)


# ---------------------------------------------------------------- geometry
def rotation(q):
    """(N, 4) quaternions (w, x, y, z) -> (N, 3, 3) rotation matrices in long
    double; column k is the box's axis k in the world."""
    q = np.asarray(q, LD).reshape(-1, 4)
    q = q / np.sqrt((q * q).sum(1))[:, None]
    w, x, y, z = q.T
    R = np.empty((len(q), 3, 3), LD)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def vertices(c, R, h):
    """(N, 8, 3): the corners c + R (+-h0, +-h1, +-h2)."""
    local = _SIGNS[None, :, :] * np.asarray(h, LD)[:, None, :]
    return np.asarray(c, LD)[:, None, :] + np.einsum("nik,nvk->nvi", R, local)


def overlap(va, vb, axis):
    """Overlap of the two vertex sets' projections on `axis` (N, 3): positive
    when the intervals overlap, the gap (negative) when they do not."""
    pa = np.einsum("nvi,ni->nv", va, axis)
    pb = np.einsum("nvi,ni->nv", vb, axis)
    return np.minimum(pa.max(1) - pb.min(1), pb.max(1) - pa.min(1))


def candidate_axes(Ra, Rb):
    """(N, 15, 3) axes and (N, 15) validity: the 3 + 3 face normals and the
    normalised edge crosses longer than the cut."""
    N = len(Ra)
    ax = np.zeros((N, 15, 3), LD)
    ok = np.ones((N, 15), bool)
    for k in range(3):
        ax[:, k] = Ra[:, :, k]
        ax[:, 3 + k] = Rb[:, :, k]
    for i in range(3):
        for j in range(3):
            c = np.cross(Ra[:, :, i], Rb[:, :, j])
            ln = np.sqrt((c * c).sum(1))
            good = ln > EDGE_CUT
            ax[:, 6 + 3 * i + j] = c / np.where(good, ln, 1)[:, None]
            ok[:, 6 + 3 * i + j] = good
    return ax, ok


def min_overlap(Ra, Rb, va, vb):
    ax, ok = candidate_axes(Ra, Rb)
    ov = np.stack([overlap(va, vb, ax[:, k]) for k in range(15)], 1)
    return np.where(ok, ov, np.inf).min(1)


def surface_dist(p, c, R, h):
    local = np.einsum("nik,ni->nk", R, np.asarray(p, LD) - np.asarray(c, LD))
    return (np.abs(local) - np.asarray(h, LD)).max(1)


def sphere_box_ref(c1, r, c2, R, h):
    """Sphere (c1, r) = geom1 against the box (c2, R, h): (hit, dist, pos,
    normal), normal from the sphere to the box."""
    c1, c2, h, r = np.asarray(c1, LD), np.asarray(c2, LD), np.asarray(h, LD), np.asarray(r, LD)
    center = np.einsum("nik,ni->nk", R, c1 - c2)
    clamped = np.clip(center, -h, h)
    nearest = clamped - center
    d = np.sqrt((nearest * nearest).sum(1))
    inside = d == 0
    nrm = nearest / np.where(inside, 1, d)[:, None]
    dist = d - r
    pos = (clamped + center + nrm * r[:, None]) / 2          # clamped point, sphere's deepest point
    # centre inside: nearest face, first minimum of +x -x +y -y +z -z
    face = np.stack([h[:, 0] - center[:, 0], h[:, 0] + center[:, 0], h[:, 1] - center[:, 1],
                     h[:, 1] + center[:, 1], h[:, 2] - center[:, 2], h[:, 2] + center[:, 2]], 1)
    kf = face.argmin(1)
    closest = face[np.arange(len(kf)), kf]
    a, s = kf // 2, np.where(kf % 2 == 0, LD(1), LD(-1))
    e = np.zeros_like(center)
    e[np.arange(len(kf)), a] = 1
    nrm_in = -s[:, None] * e
    # the face point centre + s closest e_a and the deepest point centre - s r e_a
    pos_in = center + e * (s * (closest - r) / 2)[:, None]
    dist = np.where(inside, -(closest + r), dist)
    nrm = np.where(inside[:, None], nrm_in, nrm)
    pos = np.where(inside[:, None], pos_in, pos)
    return dist <= 0, dist, np.einsum("nik,nk->ni", R, pos) + c2, np.einsum("nik,nk->ni", R, nrm)


def sphere_sphere_ref(c1, r1, c2, r2):
    c1, c2, r1, r2 = np.asarray(c1, LD), np.asarray(c2, LD), np.asarray(r1, LD), np.asarray(r2, LD)
    d = c2 - c1
    ln = np.sqrt((d * d).sum(1))
    n = d / ln[:, None]
    dist = ln - r1 - r2
    return dist <= 0, dist, c1 + n * (r1 + dist / 2)[:, None], n


# ---------------------------------------------------------------- families
def _qmul(a, b):
    aw, ax, ay, az = np.moveaxis(np.asarray(a), -1, 0)
    bw, bx, by, bz = np.moveaxis(np.asarray(b), -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _axis_angle(axis, angle):
    axis, angle = np.asarray(axis, float), np.asarray(angle, float)
    return np.concatenate([np.cos(angle / 2)[:, None], np.sin(angle / 2)[:, None] * axis], 1)


def _unit(rng, n, k):
    v = rng.normal(size=(n, k))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _box_rows(c1, q1, s1, c2, q2, s2):
    n = len(c1)
    return np.concatenate([np.ones((n, 2)), c1, q1, s1, c2, q2, s2], 1)


def _identity(n):
    return np.tile([1.0, 0, 0, 0], (n, 1))


def _centres(rng, n, spread=0.8):
    return rng.uniform(-0.2, 0.2, (n, 3)), rng.uniform(-spread, spread, (n, 3))


def random(n, seed=0):
    """n mixed pairs (sphere / box by a coin each, two random quaternions, 10 %
    with body 2's centre within 0.05 of body 1's: a sphere centre inside the
    box) followed by nine axis-aligned cube stacks: n + 9 rows."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        k1, k2 = rng.integers(0, 2, 2)
        q1, q2 = rng.normal(size=4), rng.normal(size=4)
        s1 = [.1, 0, 0] if k1 == 0 else list(rng.uniform(.1, .5, 3))
        s2 = [.1, 0, 0] if k2 == 0 else list(rng.uniform(.1, .5, 3))
        c2 = rng.uniform(-.8, .8, 3)
        if rng.random() < 0.1:
            c2 = rng.uniform(-.05, .05, 3)             # deep: sphere centre inside the box
        rows.append([k1, k2, 0, 0, 0, *(q1 / np.linalg.norm(q1)), *s1, *c2, *(q2 / np.linalg.norm(q2)), *s2])
    # axis-aligned stacks: parallel edges (skipped axes) and face-face clipping
    for dz in (0.79, 0.7, 0.5):
        for dx in (0.0, 0.3, 0.6):
            rows.append([1, 1, 0, 0, 0, 1, 0, 0, 0, .4, .4, .4, dx, 0.1, dz, 1, 0, 0, 0, .4, .4, .4])
    return np.array(rows, float)


def aligned(n, seed=0):
    rng = np.random.default_rng(seed)
    c1, c2 = _centres(rng, n)
    return _box_rows(c1, _identity(n), rng.uniform(.1, .5, (n, 3)), c2, _identity(n), rng.uniform(.1, .5, (n, 3)))


def one_axis(n, seed=0):
    """Both boxes turned about the same coordinate axis by independent angles:
    the edge axes along it are parallel, the others are not."""
    rng = np.random.default_rng(seed)
    c1, c2 = _centres(rng, n)
    axis = np.eye(3)[rng.integers(0, 3, n)]
    q1 = _axis_angle(axis, rng.uniform(0, 2 * np.pi, n))
    q2 = _axis_angle(axis, rng.uniform(0, 2 * np.pi, n))
    return _box_rows(c1, q1, rng.uniform(.1, .5, (n, 3)), c2, q2, rng.uniform(.1, .5, (n, 3)))


def quarter_turns(n, seed=0):
    """Box 2 = box 1's orientation times three random multiples of 90 degrees
    about x, y, z; box 1 the identity in the first half, random in the second."""
    rng = np.random.default_rng(seed)
    c1, c2 = _centres(rng, n)
    q1 = _identity(n)
    q1[n // 2:] = _unit(rng, n - n // 2, 4)
    turn = _identity(n)
    for a in range(3):
        turn = _qmul(turn, _axis_angle(np.tile(np.eye(3)[a], (n, 1)), rng.integers(0, 4, n) * (np.pi / 2)))
    return _box_rows(c1, q1, rng.uniform(.1, .5, (n, 3)), c2, _qmul(q1, turn), rng.uniform(.1, .5, (n, 3)))


def coincident(n, seed=0):
    """Random orientations, centre offset a random direction times one of
    0, 1e-12, 1e-3 (body 1 at the origin in the first half)."""
    rng = np.random.default_rng(seed)
    c1 = rng.uniform(-0.2, 0.2, (n, 3))
    c1[:n // 2] = 0
    off = _unit(rng, n, 3) * np.array([0.0, 1e-12, 1e-3])[rng.integers(0, 3, n)][:, None]
    return _box_rows(c1, _unit(rng, n, 4), rng.uniform(.1, .5, (n, 3)), c1 + off, _unit(rng, n, 4),
                     rng.uniform(.1, .5, (n, 3)))


def thin(n, seed=0):
    """Plates and rods: half extents 0.01, U(0.2, 0.5), U(0.01, 0.5), permuted."""
    rng = np.random.default_rng(seed)

    def sizes():
        s = np.stack([np.full(n, 0.01), rng.uniform(.2, .5, n), rng.uniform(.01, .5, n)], 1)
        return np.array([row[rng.permutation(3)] for row in s])
    c1, c2 = rng.uniform(-0.1, 0.1, (n, 3)), rng.uniform(-0.5, 0.5, (n, 3))
    return _box_rows(c1, _unit(rng, n, 4), sizes(), c2, _unit(rng, n, 4), sizes())


def near_parallel(n, seed=0):
    """q2 = q1 times a rotation by 10^U(-8, -3) rad about a random axis: edge
    pairs on both sides of the parallel-edge cut."""
    rng = np.random.default_rng(seed)
    c1, c2 = _centres(rng, n)
    q1 = _unit(rng, n, 4)
    q2 = _qmul(q1, _axis_angle(_unit(rng, n, 3), 10.0 ** rng.uniform(-8, -3, n)))
    return _box_rows(c1, q1, rng.uniform(.1, .5, (n, 3)), c2, q2, rng.uniform(.1, .5, (n, 3)))


TOUCH_DZ = (0.8, 0.8 - 1e-12, 0.8 + 1e-12, 0.79)
TOUCH_DX = (0.0, 0.8, 0.8 - 1e-12, 0.4)


def touching(n=16, seed=0):
    """Two 0.4-cubes, identity orientation, offset (dx, 0, dz): the 16 rows of
    TOUCH_DZ x TOUCH_DX (dz outer), whatever n and seed."""
    rows = [[1, 1, 0, 0, 0, 1, 0, 0, 0, .4, .4, .4, dx, 0, dz, 1, 0, 0, 0, .4, .4, .4]
            for dz in TOUCH_DZ for dx in TOUCH_DX]
    return np.array(rows, float)


FAMILIES = {"random": random, "aligned": aligned, "one_axis": one_axis, "quarter_turns": quarter_turns,
            "coincident": coincident, "thin": thin, "near_parallel": near_parallel, "touching": touching}
FACE_ONLY = ("aligned", "one_axis", "quarter_turns")
MOTION_FAMILIES = ("random", "thin")      # properties 10 and 11


# ---------------------------------------------------------------- results
class Result:
    """A kat_narrow output (N, 33) taken apart."""

    def __init__(self, out):
        out = np.asarray(out, float)
        self.out = out
        self.finite = bool(np.isfinite(out).all())
        cnt = np.nan_to_num(out[:, 0])
        self.count_ok = bool(((cnt == np.round(cnt)) & (cnt >= 0) & (cnt <= 4)).all())
        self.cnt = np.clip(cnt, 0, 4).astype(int)
        rec = np.nan_to_num(out[:, 1:]).reshape(-1, 4, 8)
        self.valid = np.arange(4)[None, :] < self.cnt[:, None]
        self.dist = rec[:, :, 0].astype(LD)
        self.pos = rec[:, :, 1:4].astype(LD)
        self.nrm = rec[:, :, 4:7].astype(LD)
        self.kind = np.where(self.valid, rec[:, :, 7], -1).astype(int)


class Report:
    """Worst residual per property, the counts of skipped and exempted cases
    and the failures that no tolerance decides."""

    def __init__(self, family, rows):
        self.family, self.rows = family, rows
        self.res, self.counts, self.fails = {}, {}, []
        self.caps = {}

    def worst(self, name, values):
        values = np.asarray(values, LD).ravel()
        v = float(values.max()) if values.size else 0.0
        self.res[name] = max(self.res.get(name, 0.0), v)

    def fail(self, cond, text):
        if cond:
            self.fails.append(text)

    def capped(self, name, values, cap):
        """Residuals of which at most cap (a count) may exceed the tolerance."""
        self.caps[name] = (np.asarray(values, LD).ravel(), int(np.floor(cap)))

    def capped_needed(self, name):
        """The tolerance this capped property needs once the allowed number
        of cases is exempted."""
        v, cap = self.caps[name]
        v = np.sort(v)[::-1]
        return float(v[cap]) if v.size > cap else 0.0

    def needed(self):
        """The tolerance at which this report would pass."""
        plain = [v for k, v in self.res.items() if k != "decision"]
        return max([self.capped_needed(k) for k in self.caps] + plain + [0.0])

    def failures(self, tol):
        bad = list(self.fails)
        bad += [f"{k}: residual {v:.3e} > tol {tol:.1e}" for k, v in self.res.items() if k != "decision" and v > tol]
        for k, (v, cap) in self.caps.items():
            miss = int((v > tol).sum())
            self.counts[k + " exempted"] = miss
            if miss > cap:
                bad.append(f"{k}: {miss} of {v.size} beyond tol {tol:.1e} (at most {cap} may be), "
                           f"worst {float(v.max()):.3e}")
        return bad

    def __str__(self):
        res = ", ".join(f"{k} {v:.2e}" for k, v in sorted(self.res.items()))
        return f"[{self.family}: {self.rows} rows; {self.counts}; residuals: {res}]"


def _split(inp):
    k = inp[:, :2].astype(int)
    return k[:, 0], k[:, 1], inp[:, 2:5], inp[:, 5:9], inp[:, 9:12], inp[:, 12:15], inp[:, 15:19], inp[:, 19:22]


def _rows(mask, limit=5):
    idx = np.nonzero(mask)[0]
    return f"{idx.size} rows, first {idx[:limit].tolist()}"


def measure(inp, out, near, family, exact_ties=True, decision=True):
    """Properties 1-9 of `out` = narrowphase(inp) against the geometry."""
    inp = np.asarray(inp, float)
    r = Result(out)
    rep = Report(family, len(inp))
    N = len(inp)
    k1, k2, c1, q1, s1, c2, q2, s2 = _split(inp)
    cnt, valid = r.cnt, r.valid
    hit = cnt > 0
    rep.counts["hit_rows"] = int(hit.sum())

    # 1, 2
    rep.fail(not r.finite, "1: an output word is not finite")
    rep.fail(not r.count_ok, "1: a count is not an integer in 0..4")
    rep.fail(bool((r.dist[valid] > 0).any()), f"2: dist > 0 ({_rows((valid & (r.dist > 0)).any(1))})")
    rep.fail(not np.isin(r.kind[valid], KINDS).all(), "2: a kind outside {16, 17, 32-35, 40}")
    rep.kinds = set(r.kind[valid].tolist())

    # 3: the kinds of a pair type, face kinds in order, one edge contact
    bb, ss = (k1 == BOX) & (k2 == BOX), (k1 == SPHERE) & (k2 == SPHERE)
    sb = ~bb & ~ss
    first = r.kind[:, 0]
    face = bb & hit & (first != 40)
    edge = bb & hit & (first == 40)
    want = np.where(valid, 32 + np.arange(4)[None, :], -1)
    rep.fail(bool((r.kind[face] != want[face]).any()),
             f"3: face kinds not 32 + t in order ({_rows(face & (r.kind != want).any(1))})")
    rep.fail(bool((cnt[edge] != 1).any()), "3: an edge result with more than one contact")
    rep.fail(bool(((cnt[sb] > 1) | (hit[sb] & (first[sb] != 17))).any()),
             "3: a sphere-box row is not one contact of kind 17")
    rep.fail(bool(((cnt[ss] > 1) | (hit[ss] & (first[ss] != 16))).any()),
             "3: a sphere-sphere row is not one contact of kind 16")
    rep.counts["face_rows"], rep.counts["edge_rows"] = int(face.sum()), int(edge.sum())

    # 5: unit normal from geom1 to geom2 (the sphere is geom1 of a sphere-box pair)
    flip = (k1 == BOX) & (k2 == SPHERE)
    g12 = np.where(flip[:, None], -1, 1) * (c2.astype(LD) - c1)
    nlen = np.sqrt((r.nrm * r.nrm).sum(2))
    rep.worst("5 |n|-1", np.abs(nlen - 1)[valid])
    rep.worst("5 n.(c2-c1)", np.maximum(0, -(r.nrm * g12[:, None, :]).sum(2))[valid])

    # box-box rows against the vertices
    b = np.nonzero(bb)[0]
    if b.size:
        Ra, Rb = rotation(q1[b]), rotation(q2[b])
        va, vb = vertices(c1[b], Ra, s1[b]), vertices(c2[b], Rb, s2[b])
        mo = min_overlap(Ra, Rb, va, vb)
        # 4
        wrong = (cnt[b] > 0) != (mo > 0)
        rep.worst("decision", np.abs(mo)[wrong])
        skipped = np.abs(mo) < near
        rep.counts["decision_skipped"] = int(skipped.sum())
        if decision:
            rep.fail(bool((wrong & ~skipped).any()),
                     f"4: contacts without overlap or overlap without contacts "
                     f"({_rows(wrong & ~skipped)} of the box rows, "
                     f"worst |min_overlap| {float(np.abs(mo)[wrong].max()) if wrong.any() else 0:.3e})")
            if family != "touching":
                rep.fail(skipped.sum() > SKIP_CAP * N,
                         f"4: {int(skipped.sum())} rows within near of touching (cap {SKIP_CAP:.0%})")
        surf = []
        for t in range(4):
            m = valid[b, t]
            n, d, p = r.nrm[b, t], r.dist[b, t], r.pos[b, t]
            # 6
            ov = overlap(va, vb, n)
            rep.worst("6 -dist<=overlap(n)", np.maximum(0, -d - ov)[m])
            rep.worst("6 overlap(n)<=1.05min", np.maximum(0, ov - EDGE_BIAS * mo)[m])
            # 7
            pp, pm = p + n * (d / 2)[:, None], p - n * (d / 2)[:, None]
            A, B = (c1[b], Ra, s1[b]), (c2[b], Rb, s2[b])
            one = np.maximum(np.abs(surface_dist(pp, *A)), np.abs(surface_dist(pm, *B)))
            two = np.maximum(np.abs(surface_dist(pp, *B)), np.abs(surface_dist(pm, *A)))
            surf.append(np.where(m, np.minimum(one, two), 0))
        surf = np.stack(surf, 1)
        is_edge = r.kind[b] == 40
        rep.worst("7 surface (face)", surf[valid[b] & ~is_edge])
        edge_surface = surf[valid[b] & is_edge]
        rep.counts["edge_contacts"] = int(edge_surface.size)
        rep.capped("7 surface (edge)", edge_surface, EDGE_MISS_CAP * edge_surface.size)
        # 9
        if family == "touching":
            dx, dz = c2[b, 0].astype(LD) - c1[b, 0], c2[b, 2].astype(LD) - c1[b, 2]
            reach = (s1[b, 2].astype(LD) + s2[b, 2].astype(LD))
            sep = np.maximum(dz - reach, dx - reach)
            asserted = np.ones(len(b), bool) if exact_ties else np.abs(sep) >= near
            expect = np.where(sep > 0, 0, 4)
            rep.fail(bool(((cnt[b] != expect) & asserted).any()),
                     f"9: counts {cnt[b].tolist()} where {expect.tolist()} follow from the definition")
            rep.worst("9 dist", np.abs(r.dist[b] - sep[:, None])[valid[b]])

    # 8: the closed forms
    for mask, ref in ((sb, "sb"), (ss, "ss")):
        s = np.nonzero(mask)[0]
        if not s.size:
            continue
        if ref == "ss":
            h, d, p, n = sphere_sphere_ref(c1[s], s1[s, 0], c2[s], s2[s, 0])
        else:
            f = flip[s][:, None]
            h, d, p, n = sphere_box_ref(np.where(f, c2[s], c1[s]), np.where(f[:, 0], s2[s, 0], s1[s, 0]),
                                        np.where(f, c1[s], c2[s]), rotation(np.where(f, q1[s], q2[s])),
                                        np.where(f, s1[s], s2[s]))
        differ = (cnt[s] > 0) != h
        rep.worst("decision", np.abs(d)[differ])
        far = differ & (np.abs(d) >= near)
        rep.fail(bool(far.any()), f"8: {ref} count differs from the closed form ({_rows(far)})")
        both = (cnt[s] > 0) & h
        rep.worst(f"8 {ref} dist", np.abs(r.dist[s, 0] - d)[both])
        rep.worst(f"8 {ref} pos", np.abs(r.pos[s, 0] - p)[both])
        rep.worst(f"8 {ref} normal", np.abs(r.nrm[s, 0] - n)[both])
    return rep


def _transformed(inp, seed):
    """Every row's two bodies moved by one random rotation and translation."""
    rng = np.random.default_rng(seed)
    g = _unit(rng, 1, 4)
    t = rng.uniform(-1, 1, 3)
    Q = rotation(g)[0]
    out = np.array(inp, float)
    for c, q in ((slice(2, 5), slice(5, 9)), (slice(12, 15), slice(15, 19))):
        out[:, c] = (np.asarray(inp[:, c], LD) @ Q.T + t).astype(float)
        out[:, q] = _qmul(np.asarray(g, LD), np.asarray(inp[:, q], LD)).astype(float)
    return out, Q, np.asarray(t, LD)


def measure_motion(inp, out, narrow, rep, seed=12345):
    """Properties 10 (rigid-motion covariance) and 11 (swap symmetry) of the
    narrowphase `narrow` whose result on inp is out, added to rep."""
    inp = np.asarray(inp, float)
    a = Result(out)
    with_contacts = int((a.cnt > 0).sum())
    # 10
    inp2, Q, t = _transformed(inp, seed)
    b = Result(narrow(inp2))
    differ = (a.cnt != b.cnt) | (a.kind != b.kind).any(1)
    rep.counts["covariance_mismatches"] = int(differ.sum())
    rep.fail(differ.sum() > MISMATCH_CAP * with_contacts,
             f"10: count or kinds change under a rigid motion in {_rows(differ)} of {with_contacts} with contacts")
    m = a.valid & ~differ[:, None]
    rep.worst("10 dist", np.abs(b.dist - a.dist)[m])
    rep.worst("10 pos", np.abs(b.pos - (a.pos @ Q.T + t))[m])
    rep.worst("10 normal", np.abs(b.nrm - a.nrm @ Q.T)[m])
    # 11
    bb = np.nonzero((inp[:, 0] == BOX) & (inp[:, 1] == BOX))[0]
    sw = inp[bb][:, [1, 0] + list(range(12, 22)) + list(range(2, 12))]
    s = Result(narrow(sw))
    ca, va = a.cnt[bb], a.valid[bb]
    differ = ca != s.cnt
    with_contacts = int(((ca > 0) | (s.cnt > 0)).sum())
    rep.counts["swap_count_mismatches"] = int(differ.sum())
    rec_a = np.concatenate([a.dist[bb][..., None], a.pos[bb], a.nrm[bb]], 2)
    rec_s = np.concatenate([s.dist[..., None], s.pos, -s.nrm], 2)
    err = np.abs(rec_a[:, :, None, :] - rec_s[:, None, :, :]).max(3)          # [row, contact of a, contact of s]
    err = np.where(va[:, :, None] & s.valid[:, None, :], err, np.inf)
    row = np.maximum(np.where(va, err.min(2), 0).max(1), np.where(s.valid, err.min(1), 0).max(1))
    rep.capped("11 swap", np.where(differ, np.inf, row)[(ca > 0) | (s.cnt > 0)], MISMATCH_CAP * with_contacts)
    return rep


def reach_failures(rep):
    """Did the family reach what it is for?"""
    f, c, bad = rep.family, rep.counts, []
    if f == "random" and not set(KINDS) <= rep.kinds:
        bad.append(f"random shows only the kinds {sorted(rep.kinds)}")
    if f in FACE_ONLY and not (c["hit_rows"] > 150 and c["edge_rows"] == 0):
        bad.append(f"{f}: {c['hit_rows']} hit rows (want > 150), {c['edge_rows']} of them edge results (want 0)")
    if f == "coincident" and c["hit_rows"] != rep.rows:
        bad.append(f"coincident: only {c['hit_rows']} of {rep.rows} rows hit")
    if f == "thin" and not (c["face_rows"] and c["edge_rows"]):
        bad.append("thin shows no face or no edge result")
    if f in MOTION_FAMILIES and c["edge_contacts"] < 100:
        bad.append(f"{f}: {c['edge_contacts']} edge contacts, the 2 % cap needs at least 100")
    return bad


def assert_properties(inp, out, family, dtype="f64", narrow=None):
    """Every property of part 2 on out = narrowphase(inp), with the bounds of
    dtype; narrow (the narrowphase itself) adds properties 10 and 11 on the
    families they are for.  Returns the report."""
    rep = measure(inp, out, NEAR[dtype], family, exact_ties=dtype == "f64",
                  decision=not (dtype == "f32" and family in F32_NO_DECISION))
    if narrow is not None and family in MOTION_FAMILIES:
        measure_motion(inp, out, narrow, rep)
    bad = rep.failures(TOL[dtype]) + reach_failures(rep)
    assert not bad, "\n".join(bad) + f"\n{rep}"
    return rep


# ---------------------------------------------------------------- a world of pairs
def lattice_rows(n=600, spacing=8.0):
    """n rows drawn from all families (the 16 of `touching`, the rest shared
    evenly, the remainder from `random`), interleaved, each pair moved to its
    own point of a square lattice.  A pair reaches at most 0.2 + 0.8 sqrt(3)
    + 0.5 sqrt(3) < 2.5 from its lattice point, so at `spacing` 8 no two
    pairs' bounding spheres overlap.  Sphere-box pairs alternate between
    sphere first and box first."""
    per = (n - 16) // 7
    parts = [touching()]
    for f in FAMILIES:
        if f != "touching":
            parts.append(FAMILIES[f](1000, CASES[f][1])[:per + (n - 16 - 7 * per if f == "random" else 0)])
    rows = np.concatenate(parts)
    rows = rows[np.random.default_rng(7).permutation(len(rows))]
    mixed = np.nonzero(rows[:, 0] != rows[:, 1])[0]
    for j, r in enumerate(mixed):
        if rows[r, 0] != (BOX if j % 2 == 0 else SPHERE):
            rows[r] = rows[r][[1, 0] + list(range(12, 22)) + list(range(2, 12))]
    side = int(np.ceil(np.sqrt(len(rows))))
    at = np.stack([spacing * (np.arange(len(rows)) % side), spacing * (np.arange(len(rows)) // side),
                   np.zeros(len(rows))], 1)
    rows[:, 2:5] += at
    rows[:, 12:15] += at
    return rows


def pair_scene(rows):
    """One Scene of 2 len(rows) bodies at rest: row p's bodies get the ids 2p
    and 2p + 1.  No gravity, one plane far below."""
    from rbhip import scenes
    n = len(rows)
    kind = rows[:, :2].astype(np.int32).reshape(2 * n)
    size = rows[:, [9, 10, 11, 19, 20, 21]].reshape(2 * n, 3)
    qpos = np.concatenate([rows[:, 2:9], rows[:, 12:19]], 1).reshape(2 * n, 7)
    box = kind == BOX
    mass = np.where(box, scenes.M_CUBE_H04, scenes.M_SPHERE_R01)
    inertia = np.where(box, scenes.I_CUBE_H04, scenes.I_SPHERE_R01)[:, None] * np.ones((1, 3))
    return scenes.Scene("pair_lattice", kind, mass, inertia, size, np.array([[0.0, 0, 1, 0, 0, -100.0]]), qpos,
                        np.zeros((2 * n, 6)), dt=0.01, restitution=0.5, friction=0.4, threshold=0.0,
                        gravity=np.zeros(3))


def assert_records_are_the_narrowphase(records, expect):
    """Both bodies of every pair carry the pair's narrowphase result: records
    = (counts, partner, kind, dist) of one step of pair_scene(rows), expect =
    kat_narrow(rows)."""
    cnt, par, kin, dis = records
    start = np.concatenate([[0], np.cumsum(cnt)])
    bad = []
    for p in range(len(expect)):
        nc = int(expect[p, 0])
        kinds, dist = expect[p, 8:8 + 8 * nc:8].astype(np.int32), expect[p, 1:1 + 8 * nc:8]
        for body, other in ((2 * p, 2 * p + 1), (2 * p + 1, 2 * p)):
            lo, hi = start[body], start[body + 1]
            if not (hi - lo == nc and np.array_equal(kin[lo:hi], kinds) and (par[lo:hi] == other).all()
                    and np.array_equal(np.ascontiguousarray(dis[lo:hi]).view(np.uint64), dist.view(np.uint64))):
                bad.append(body)
    assert not bad, f"{len(bad)} bodies' records differ from the narrowphase of their pair, first {bad[:5]}"
