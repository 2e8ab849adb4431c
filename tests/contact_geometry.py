"""A plain geometric reference for contact generation, and the properties a
contact list must have.  Shared by tests/test_oracle_contact_geometry.py (the
CPU oracle) and tests/test_gpu_contact_geometry.py (the device: the batch
query, and a World in every step form).

The plane and sphere primitives and the assembly of a body's list (which
pairs are found, their order, which body is geom1, the four-corner cap) exist
three times in this project: tests/golden/make_golden.py, oracle/
rb_oracle_impl.h and csrc/rb_device.hpp / rb_grid.hpp.  The three were written
from one description, so a mistake in that description passes every golden and
every device-vs-oracle comparison.  This module is the outside anchor (DESIGN
§2.6): NumPy long double, all pairs, working from vertex coordinates and
signed point-plane distances only.  It has no cells, no `ldist`, no
`s = -dist / 2 - r`: it shares no structure with the code it judges.

  Problem                  G environments of M bodies, planes per environment
  reference_lists(pb)      per body: every plane's signed gap (spheres) or the
                           8 vertices' signed distances and offset distances
                           (boxes); every other body of the environment within
                           reach, ascending id, with its gap
  measure / assert_properties   the properties of a result in the CSR shape of
                           oracle.contacts(): (counts, partner, kind, dist[, pos, frame])

Properties (numbering as in DESIGN §2.6):
  1 every word finite; a body's records ordered: planes ascending as -1 - p,
    then partners by ascending id; plane-box kinds 1 + corner ascending within
    a plane, at most 4 per plane
  2 plane-sphere: a record iff gap <= 0; dist = gap; frame = the normal;
    pos + frame dist / 2 on the sphere, pos - frame dist / 2 on the plane
  3 plane-box: the listed corners are the first four, in bit order, of the
    vertices with signed distance <= 0 and offset distance <= 0; dist = the
    vertex's signed distance; pos + frame dist / 2 = the vertex;
    pos - frame dist / 2 on the plane; frame = the normal
  4 sphere-sphere: a record on both bodies iff centre distance - r1 - r2 <= 0;
    dist bit-equal on both; frame the unit vector from the lower id to the
    higher ((1, 0, 0) for coincident centres); pos -+ frame dist / 2 one on
    each sphere
  5 box-involved partners: every listed one's bounding spheres overlap (the
    converse cannot be read from records: a partner whose narrowphase finds no
    contact leaves none; its records stay with box_geometry)

A decision within `near` of its threshold is free.  The statements are one-
sided: every listed item passes its test within near; every clearly passing
item is listed (a corner: unless four listed ones precede it on that plane);
every value is right.  On a body all of whose decisions are clear they are
the strict statements above.  A body with a decision within near is counted,
and in the random families at most 1 % of the bodies may be (NEAR_CAP): a
condition, not a measurement.  The degenerate families carry the record count
each body must have (Problem.expect; offsets of 0 and +-2^-40 on exactly
representable operands, so the outcome follows from the definition with no
rounding: hit, hit, miss), asserted in fp64.

Bounds.  fp64: tol 1e-12, near 1e-9, as in box_geometry.  The oracle's worst
residual over all families at CASES is 4.55e-13 (property 4, pos on the
spheres, in cells_period, whose coordinates reach 6.6e3: half an ulp of pos
there is 4.5e-13; every family within 40 m of the origin stays below 4e-15).

fp32: measured, not guessed.  The properties were run on the oracle's fp32
restatement (oracle.contacts(..., dtype="f32")) on inputs rounded to fp32
first, over all families at CASES.  F32_MEASURED has the worst residual of
each property; the worst of all is 3.815e-6 (property 4, pos on the spheres,
in cells_period at 103 m from the origin, where half an ulp of pos is
3.8e-6), and tol is 8 x that, 3.06e-5: the factor covers inputs other than
these seeds.  The largest gap at which a decision differed from long double
is 3.62e-8 (pairs_grazing), so near is the smallest power of ten above
8 x 3.62e-8 = 2.9e-7: 1e-6.  The fp32 families stay within 108 m of the
origin: cells_period with k <= 8 shifts a cluster by 0.4004 x 2^8 = 102.5,
every other family stays within 40 m.

Observed shares on the oracle: bodies with a decision within near, of the
bodies of the family at CASES.  The families under the cap (RANDOM_FAMILIES):
plane_random 0 of 2,000, plane_deep 0 of 1,000 (fp32: 1), pairs_random 0 of
2,000, cells_negative 0 of 1,100, radius_mix 0 of 1,098, in both precisions.
The built ones: plane_diagonal 1,263 of 2,000 (centres on the plane),
plane_flat 9 of 9, plane_spheres 656 of 1,000, pairs_grazing 1,462 of 1,806
(fp32: 192, whose band is 1e-4 wide), and none in pairs_coincident,
cells_lattice, cells_half and cells_period.  1,302 of plane_diagonal's 4,000
box-plane rows have more than four passing corners.  The tile-shaped families
(TILE_FAMILIES: the broadphase edges thin in z, which the tile form commits):
none in sheet_lattice (1,100), sheet_negative (406), sheet_period (1,080),
sheet_radius (1,098) and sheet_piles (1,486), in both precisions;
sheet_negative and sheet_radius are under the cap.

The tests can fail: of four mutants of the oracle, built apart from the tree,
three fail tests/test_oracle_contact_geometry.py and the fourth is equivalent
(its docstring and DESIGN §2.6 have the table).
"""
import numpy as np

from box_geometry import LD, Report, rotation

SPHERE, BOX = 0, 1
MAX_PLANES = 8
BOX_PAIR_KINDS = (17, 32, 33, 34, 35, 40)

TOL = {"f64": 1e-12, "f32": 3.06e-5}    # f32: 8 x the worst of F32_MEASURED
NEAR = {"f64": 1e-9, "f32": 1e-6}       # f32: the power of ten above 8 x F32_MEASURED["decision"]
NEAR_CAP = 0.01
KEEP = 1e-3                             # pairs with a gap up to this are kept in the reference

# Worst residual of each property on the oracle's fp32 restatement over CASES
# ("decision": the largest |gap| at which a decision differed from long double).
F32_MEASURED = {"2 dist": 3.592e-8, "2 frame": 0.0, "2 on plane": 1.34e-7, "2 on sphere": 1.172e-7,
                "3 dist": 3.406e-7, "3 frame": 0.0, "3 on plane": 4.294e-7, "3 vertex": 4.371e-7,
                "4 dist": 1.265e-7, "4 frame": 1.428e-7, "4 on spheres": 3.815e-6, "decision": 3.62e-8}

_BITS = np.array([[1 if i & 1 else -1, 1 if i & 2 else -1, 1 if i & 4 else -1] for i in range(8)], LD)


# ---------------------------------------------------------------- problems
class Problem:
    """G environments of M bodies each (flat arrays of N = G M bodies, body b
    of environment g at g M + b) and the planes of every environment
    (G, P, 6): normal xyz, point xyz.  expect: the record count each body must
    have, -1 where the family does not state one."""

    def __init__(self, name, M, kind, size, qpos, planes, expect=None, max_partners=16):
        self.name, self.M = name, int(M)
        self.kind = np.ascontiguousarray(kind, np.int32)
        self.size = np.ascontiguousarray(size, np.float64)
        self.qpos = np.ascontiguousarray(qpos, np.float64)
        self.planes = np.ascontiguousarray(planes, np.float64)
        self.N = self.kind.shape[0]
        self.G = self.N // self.M
        assert self.G * self.M == self.N and self.planes.shape[0] == self.G and self.planes.shape[2] == 6
        self.P = self.planes.shape[1]
        self.expect = None if expect is None else np.asarray(expect, np.int64)
        self.max_partners = max_partners

    def rounded(self):
        """The same problem with every input rounded to fp32."""
        f = lambda a: a.astype(np.float32).astype(np.float64)         # noqa: E731
        pb = Problem(self.name, self.M, self.kind, f(self.size), f(self.qpos), f(self.planes), self.expect,
                     self.max_partners)
        for k in ("graze", "inside", "axis"):            # what a family says about its own rows
            if hasattr(self, k):
                setattr(pb, k, getattr(self, k))
        return pb

    def only(self, g):
        """Environment g as a problem of its own."""
        s = slice(g * self.M, (g + 1) * self.M)
        return Problem(self.name, self.M, self.kind[s], self.size[s], self.qpos[s], self.planes[g:g + 1],
                       None if self.expect is None else self.expect[s], self.max_partners)

    def scene(self, g=0):
        """Environment g as a Scene at rest without gravity."""
        from rbhip import scenes
        s = slice(g * self.M, (g + 1) * self.M)
        return scenes.Scene(self.name, self.kind[s], np.ones(self.M), np.ones((self.M, 3)), self.size[s],
                            self.planes[g], self.qpos[s], np.zeros((self.M, 6)), dt=0.01, restitution=0.5,
                            friction=0.4, threshold=0.0, gravity=np.zeros(3))

    def scenes(self):
        return [self.scene(g) for g in range(self.G)]


def oracle_lists(oracle, pb, dtype="f64"):
    """oracle.contacts of every environment, concatenated to one CSR result
    over the problem's N bodies (partners stay ids within the environment)."""
    parts = [oracle.contacts(oracle.OracleScene(pb.scene(g), max_partners=pb.max_partners),
                             pb.qpos[g * pb.M:(g + 1) * pb.M], dtype=dtype) for g in range(pb.G)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(6))


def dense_lists(con, fields=("partner", "kind", "dist", "pos", "frame")):
    """A BatchContacts (host arrays, nothing truncated) as one CSR result."""
    cnt = np.asarray(con.counts).reshape(-1)
    assert cnt.min() >= 0 and cnt.max() <= con.max_records, (cnt.min(), cnt.max(), con.max_records)
    keep = (np.arange(con.max_records)[None, :] < cnt[:, None])
    out = [cnt.astype(np.int32)]
    for f in fields:
        a = getattr(con, f)
        out.append(None if a is None else np.asarray(a).reshape((cnt.size, con.max_records) + np.shape(a)[3:])[keep])
    return tuple(out)


# ---------------------------------------------------------------- the reference
class Ref:
    pass


def _corners(pb):
    """(N, 8, 3): vertex i of a box is c + R (+-h0, +-h1, +-h2), the sign of
    axis k positive where bit k of i is set."""
    R = rotation(pb.qpos[:, 3:7])
    local = _BITS[None, :, :] * pb.size.astype(LD)[:, None, :]
    off = np.einsum("nik,nvk->nvi", R, local)
    return pb.qpos[:, None, :3].astype(LD) + off, off


def reference_lists(pb):
    """The long-double all-pairs reference of a Problem.

    gap (N, P): (c - pp).n - r of a sphere against every plane of its
    environment (nan for a box); vdist, voff (N, P, 8): the signed distances
    (v - pp).n of a box's vertices and of the vertex offsets (v - c).n (nan
    for a sphere); pi, pj, pgap, pbox: every ordered pair of bodies of one
    environment with a gap up to KEEP, sorted by (i, j), as global ids: the
    centre distance minus the radii, or minus the bounding radii when a box is
    involved (pbox)."""
    r = Ref()
    N, M, P = pb.N, pb.M, pb.P
    box = pb.kind == BOX
    c = pb.qpos[:, :3].astype(LD)
    pl = np.repeat(pb.planes.astype(LD), M, axis=0)                  # (N, P, 6)
    n, pp = pl[:, :, :3], pl[:, :, 3:]
    rad = np.where(box, np.sqrt((pb.size.astype(LD) ** 2).sum(1)), pb.size[:, 0].astype(LD))
    r.c, r.n, r.pp, r.box = c, n, pp, box
    r.radius = pb.size[:, 0].astype(LD)
    r.bound = rad
    r.gap = np.where(box[:, None], np.nan, ((c[:, None, :] - pp) * n).sum(2) - r.radius[:, None])
    verts, off = _corners(pb)
    r.verts = verts
    vd = ((verts[:, None, :, :] - pp[:, :, None, :]) * n[:, :, None, :]).sum(3)
    vo = (off[:, None, :, :] * n[:, :, None, :]).sum(3)
    r.vdist = np.where(box[:, None, None], vd, np.nan)
    r.voff = np.where(box[:, None, None], vo, np.nan)
    # all pairs of an environment, in blocks
    pi, pj, pg = [], [], []
    gstep = max(1, (1 << 18) // (M * M))
    rstep = M if M <= 512 else 128
    for g0 in range(0, pb.G, gstep):
        g1 = min(pb.G, g0 + gstep)
        cg = c[g0 * M:g1 * M].reshape(-1, M, 3)
        rg = rad[g0 * M:g1 * M].reshape(-1, M)
        for r0 in range(0, M, rstep):
            d = cg[:, r0:r0 + rstep, None, :] - cg[:, None, :, :]
            gap = np.sqrt((d * d).sum(3)) - rg[:, r0:r0 + rstep, None] - rg[:, None, :]
            gi, ri, rj = np.nonzero(gap <= KEEP)
            keep = ri + r0 != rj
            gi, ri, rj = gi[keep], ri[keep], rj[keep]
            pi.append((g0 + gi) * M + r0 + ri)
            pj.append((g0 + gi) * M + rj)
            pg.append(gap[gi, ri, rj])
    r.pi, r.pj, r.pgap = np.concatenate(pi), np.concatenate(pj), np.concatenate(pg)
    order = np.lexsort((r.pj, r.pi))
    r.pi, r.pj, r.pgap = r.pi[order], r.pj[order], r.pgap[order]
    r.pbox = box[r.pi] | box[r.pj]
    r.pb = pb
    return r


# ---------------------------------------------------------------- the properties
def _where(mask, limit=5):
    idx = np.nonzero(mask)[0]
    return f"{idx.size}, first {idx[:limit].tolist()}"


def _len(v):
    return np.sqrt((v * v).sum(-1))


def measure(lists, ref, near):
    """The properties of `lists` = (counts, partner, kind, dist[, pos, frame])
    against ref = reference_lists(problem).  Returns a Report; its counts hold
    what the family tests ask about (near_bodies, many_corner_rows, ...)."""
    pb = ref.pb
    N, M, P = pb.N, pb.M, pb.P
    cnt, par, kin, dis = (np.asarray(a) for a in lists[:4])
    pos = None if len(lists) < 6 or lists[4] is None else np.asarray(lists[4], LD)
    frm = None if len(lists) < 6 or lists[5] is None else np.asarray(lists[5], LD)
    rep = Report(pb.name, N)
    T = int(cnt.sum())
    rep.fail(not (cnt.shape == (N,) and (cnt >= 0).all() and par.shape == (T,) and kin.shape == (T,)
                  and dis.shape == (T,)), "1: the counts do not describe the records")
    if rep.fails:
        return rep
    fin = np.isfinite(dis).all() and (pos is None or (np.isfinite(pos).all() and np.isfinite(frm).all()))
    rep.fail(not fin, "1: a word is not finite")
    dis = np.nan_to_num(dis).astype(LD)
    owner = np.repeat(np.arange(N), cnt)
    par = par.astype(np.int64)
    ok = ((par >= -P) & (par < M) & (par != owner % M))
    rep.fail(not ok.all(), f"1: a partner is no plane and no other body of the environment ({_where(~ok)})")
    if not ok.all():
        return rep
    plane = par < 0
    p_of = np.where(plane, -1 - par, 0)
    other = np.where(plane, owner, (owner // M) * M + par)
    obox = ref.box[owner]
    ps, pbx = plane & ~obox, plane & obox
    ss = ~plane & ~obox & ~ref.box[other]
    bx = ~plane & ~ss
    # 1: kinds and order
    rep.fail(bool((kin[ps] != 0).any()), "1: a plane-sphere record's kind is not 0")
    rep.fail(bool(((kin[pbx] < 1) | (kin[pbx] > 8)).any()), "1: a plane-box record's kind is not 1 + corner")
    rep.fail(bool((kin[ss] != 16).any()), "1: a sphere-sphere record's kind is not 16")
    rep.fail(not np.isin(kin[bx], BOX_PAIR_KINDS).all(), "1: a box-involved record's kind")
    if rep.fails:
        return rep
    key = np.where(plane, p_of, P + par)
    same = owner[1:] == owner[:-1]
    rep.fail(bool((same & (key[1:] < key[:-1])).any()),
             f"1: records out of order (planes as -1 - p ascending, then partners ascending) "
             f"({_where(same & (key[1:] < key[:-1]))})")
    eq = same & (key[1:] == key[:-1])
    rep.fail(bool((eq & (ps | ss)[1:]).any()), "1: a plane or a sphere partner listed twice on one sphere")
    rep.fail(bool((eq & pbx[1:] & (kin[1:] <= kin[:-1])).any()), "1: plane-box corners not ascending within a plane")
    corner_count = np.zeros((N, P), np.int64)
    np.add.at(corner_count, (owner[pbx], p_of[pbx]), 1)
    rep.fail(bool((corner_count > 4).any()), "1: more than 4 corners on one plane")
    pair_count = np.zeros(N * M, np.int64)
    np.add.at(pair_count, owner[bx] * M + par[bx], 1)
    rep.fail(bool((pair_count > 4).any()), "1: more than 4 records of one box-involved pair")
    if rep.fails:
        return rep
    unclear = np.zeros(N, bool)
    decision = [LD(0)]

    # 2: plane-sphere
    gap = ref.gap
    listed = np.zeros((N, P), bool)
    listed[owner[ps], p_of[ps]] = True
    sph = ~ref.box[:, None] & np.ones((1, P), bool)
    bad = sph & listed & (gap > near)
    rep.fail(bool(bad.any()), f"2: a sphere listed on a plane it clears (bodies {_where(bad.any(1))}, "
                              f"worst gap {float(np.nanmax(np.where(bad, gap, -np.inf))):.3e})")
    bad = sph & ~listed & (gap <= -near)
    rep.fail(bool(bad.any()), f"2: a sphere not listed on a plane it touches (bodies {_where(bad.any(1))}, "
                              f"worst gap {float(np.nanmin(np.where(bad, gap, np.inf))):.3e})")
    decision.append(np.abs(gap[sph & (listed != (gap <= 0))]))
    unclear |= (sph & (np.abs(gap) < near)).any(1)
    o, p = owner[ps], p_of[ps]
    rep.worst("2 dist", np.abs(dis[ps] - gap[o, p]))
    if pos is not None:
        nn = ref.n[o, p]
        rep.worst("2 frame", np.abs(frm[ps] - nn))
        half = (dis[ps] / 2)[:, None]
        rep.worst("2 on sphere", np.abs(_len(pos[ps] + frm[ps] * half - ref.c[o]) - ref.radius[o]))
        rep.worst("2 on plane", np.abs(((pos[ps] - frm[ps] * half - ref.pp[o, p]) * nn).sum(1)))

    # 3: plane-box
    vd, vo = ref.vdist, ref.voff
    isb = ref.box[:, None, None] & np.ones((1, P, 8), bool)
    lc = np.zeros((N, P, 8), bool)
    lc[owner[pbx], p_of[pbx], kin[pbx] - 1] = True
    passing = isb & (vd <= 0) & (vo <= 0)
    clear_pass = isb & (vd <= -near) & (vo <= -near)
    clear_fail = isb & ((vd >= near) | (vo >= near))
    bad = lc & clear_fail
    rep.fail(bool(bad.any()), f"3: a listed corner clearly fails signed distance <= 0 or offset distance <= 0 "
                              f"(bodies {_where(bad.any((1, 2)))})")
    before = np.cumsum(lc, axis=2) - lc                              # listed corners preceding each vertex
    bad = clear_pass & ~lc & (before < 4)
    rep.fail(bool(bad.any()), f"3: a clearly passing corner is not listed though fewer than four precede it "
                              f"(bodies {_where(bad.any((1, 2)))})")
    with np.errstate(invalid="ignore"):
        wrong_in = lc & ~passing
        wrong_out = passing & ~lc & (before < 4)
        decision.append(np.maximum(vd, vo)[wrong_in])
        decision.append(np.minimum(-vd, -vo)[wrong_out])
    unclear |= (isb & ~clear_pass & ~clear_fail).any((1, 2))
    rep.counts["box_plane_rows"] = int(ref.box.sum()) * P
    rep.counts["many_corner_rows"] = int((passing.sum(2) > 4).sum())
    rep.counts["corner_records"] = int(pbx.sum())
    o, p, v = owner[pbx], p_of[pbx], kin[pbx] - 1
    rep.worst("3 dist", np.abs(dis[pbx] - vd[o, p, v]))
    if pos is not None:
        nn = ref.n[o, p]
        rep.worst("3 frame", np.abs(frm[pbx] - nn))
        half = (dis[pbx] / 2)[:, None]
        rep.worst("3 vertex", np.abs(pos[pbx] + frm[pbx] * half - ref.verts[o, v]))
        rep.worst("3 on plane", np.abs(((pos[pbx] - frm[pbx] * half - ref.pp[o, p]) * nn).sum(1)))

    # 4: sphere-sphere
    o, j = owner[ss], other[ss]
    g_rec = _len(ref.c[j] - ref.c[o]) - ref.radius[o] - ref.radius[j]
    bad = g_rec > near
    rep.fail(bool(bad.any()), f"4: a listed pair of spheres is apart ({_where(bad)} of the sphere-sphere records, "
                              f"worst gap {float(g_rec.max()) if g_rec.size else 0:.3e})")
    keys = o * N + j
    cand = ~ref.pbox
    ckeys = ref.pi[cand] * N + ref.pj[cand]
    cgap = ref.pgap[cand]
    have = np.isin(ckeys, keys)
    bad = ~have & (cgap <= -near)
    rep.fail(bool(bad.any()), f"4: an overlapping pair of spheres is not listed (bodies "
                              f"{np.unique(ref.pi[cand][bad])[:6].tolist()}, {int(bad.sum())} records missing, "
                              f"deepest gap {float(cgap[bad].min()) if bad.any() else 0:.3e})")
    decision.append(np.abs(cgap[have != (cgap <= 0)]))
    decision.append(np.abs(g_rec[g_rec > 0]))
    near_pair = cand & (np.abs(ref.pgap) < near)
    unclear[ref.pi[near_pair]] = True
    rep.counts["sphere_pairs"] = int((cgap <= 0).sum()) // 2
    rep.counts["ss_records"] = int(ss.sum())
    # the partner's record of the same pair: present, dist bit-equal
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    at = np.searchsorted(sk, j * N + o)
    found = (at < sk.size) & (sk[np.minimum(at, max(sk.size - 1, 0))] == j * N + o) if sk.size else np.zeros(0, bool)
    bad = ~found & (np.abs(g_rec) >= near)
    rep.fail(bool(bad.any()), f"4: a pair listed on one body only ({_where(bad)})")
    mate = order[np.minimum(at, max(sk.size - 1, 0))] if sk.size else at
    d_ss = dis[ss]
    rep.fail(bool((found & (d_ss != d_ss[mate])).any()), "4: dist differs between the two bodies of a pair")
    rep.worst("4 dist", np.abs(d_ss - g_rec))
    if pos is not None:
        lo, hi = np.minimum(o, j), np.maximum(o, j)
        d = ref.c[hi] - ref.c[lo]
        ln = _len(d)
        unit = np.where((ln == 0)[:, None], np.array([1, 0, 0], LD), d / np.where(ln == 0, 1, ln)[:, None])
        rep.worst("4 frame", np.abs(frm[ss] - unit))
        half = (d_ss / 2)[:, None]
        rep.worst("4 on spheres", np.maximum(np.abs(_len(pos[ss] - frm[ss] * half - ref.c[lo]) - ref.radius[lo]),
                                             np.abs(_len(pos[ss] + frm[ss] * half - ref.c[hi]) - ref.radius[hi])))
        rep.counts["coincident_records"] = int((ln == 0).sum())

    # 5: box-involved partners
    o, j = owner[bx], other[bx]
    g_box = _len(ref.c[j] - ref.c[o]) - ref.bound[o] - ref.bound[j]
    rep.fail(bool((g_box > near).any()), f"5: a listed box-involved partner's bounding sphere is apart ({_where(g_box > near)})")
    rep.counts["box_pair_records"] = int(bx.sum())
    near_pair = ref.pbox & (np.abs(ref.pgap) < near)
    unclear[ref.pi[near_pair]] = True

    rep.unclear = unclear
    rep.counts["near_bodies"] = int(unclear.sum())
    rep.res["decision"] = float(max([float(np.max(x)) for x in decision if np.size(x)] + [0.0]))
    # the degenerate families' stated outcome
    if pb.expect is not None:
        rep.expect_bad = np.nonzero((pb.expect >= 0) & (cnt != pb.expect))[0]
    return rep


def assert_properties(lists, pb, dtype="f64", ref=None):
    """Every property on `lists`, a result for the Problem pb, with the bounds
    of dtype (for fp32 pb is the rounded problem).  Returns the report."""
    ref = reference_lists(pb) if ref is None else ref
    rep = measure(lists, ref, NEAR[dtype])
    bad = rep.failures(TOL[dtype])
    if not rep.fails:
        if pb.name in RANDOM_FAMILIES and rep.counts["near_bodies"] > NEAR_CAP * pb.N:
            bad.append(f"{rep.counts['near_bodies']} of {pb.N} bodies have a decision within near (cap {NEAR_CAP:.0%})")
        if pb.expect is not None and dtype == "f64" and rep.expect_bad.size:
            bad.append(f"{rep.expect_bad.size} bodies' record counts differ from what the definition gives, "
                       f"first {rep.expect_bad[:6].tolist()}")
    assert not bad, "\n".join(bad) + f"\n{rep}"
    return rep


# ---------------------------------------------------------------- families
def _unit(rng, n, k=3):
    v = rng.normal(size=(n, k))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _ident(n):
    return np.tile([1.0, 0, 0, 0], (n, 1))


def _qpos(c, q):
    return np.concatenate([np.asarray(c, float), np.asarray(q, float)], 1)


def _tangent_frame(n1, n2):
    """Unit t orthogonal to both normals."""
    t = np.cross(n1, n2)
    if np.linalg.norm(t) < 1e-6:
        t = np.cross(n1, [1.0, 0, 0] if abs(n1[0]) < 0.9 else [0, 1.0, 0])
    return t / np.linalg.norm(t)


SLOT = 4.0          # spacing of an environment's sphere pairs along x
PLANE_SLOT = 2.0    # spacing of an environment's bodies along the planes' common tangent (bounding radii < 0.87)


def _place(normals, dists, M, rng):
    """Centres and planes of G environments: environment g has the normals
    normals[g] (P, 3); body b must lie at the signed centre distances
    dists[g, b] (P,) from them.  M = 1: any number of planes, the centre is
    random in [-2, 2]^3 and each plane is put where the distance asks.  M > 1:
    P <= 2, the planes pass through a random point and the bodies are spaced
    PLANE_SLOT apart along the direction both planes contain."""
    G, P = normals.shape[:2]
    c = np.zeros((G, M, 3))
    planes = np.zeros((G, P, 6))
    planes[:, :, :3] = normals
    for g in range(G):
        if M == 1:
            c[g, 0] = rng.uniform(-2, 2, 3)
            planes[g, :, 3:] = c[g, 0] - normals[g] * dists[g, 0][:, None]
            continue
        assert P <= 2
        O = rng.uniform(-2, 2, 3)
        planes[g, :, 3:] = O
        n = normals[g]
        t = _tangent_frame(n[0], n[-1])
        gram = n @ n.T
        for b in range(M):
            alpha = np.linalg.lstsq(gram, dists[g, b], rcond=None)[0]
            c[g, b] = O + alpha @ n + (b - M // 2) * PLANE_SLOT * t
    return c.reshape(G * M, 3), planes


def _plane_family(name, n, M, rng, normals, kind, size, quat, dists, expect=None):
    G = n // M
    c, planes = _place(normals[:G], dists.reshape(-1, *dists.shape[-1:])[:G * M].reshape(G, M, -1), M, rng)
    return Problem(name, M, kind[:G * M], size[:G * M], _qpos(c, quat[:G * M]), planes, expect)


def _random_normals(rng, G, P):
    return _unit(rng, G * P).reshape(G, P, 3)


def _reach(size, box):
    return np.where(box, np.linalg.norm(size, axis=1), size[:, 0])


def plane_random(n, seed=0, M=1):
    """Random unit normals (MAX_PLANES planes per body at M = 1, two per
    environment otherwise), random quaternions and half extents, spheres and
    boxes mixed (body b of every environment has the same kind), centre
    distances within +-1.2 bounding radii."""
    rng = np.random.default_rng(seed)
    G, P = n // M, (MAX_PLANES if M == 1 else 2)
    kind = np.tile(rng.integers(0, 2, M) if M > 1 else [BOX], G).astype(np.int32)
    size = rng.uniform(0.1, 0.5, (G * M, 3))
    size[kind == SPHERE, 1:] = 0
    dists = rng.uniform(-1.2, 1.2, (G * M, P)) * _reach(size, kind == BOX)[:, None]
    return _plane_family("plane_random", n, M, rng, _random_normals(rng, G, P), kind, size, _unit(rng, G * M, 4), dists)


_DIAGONALS = np.array([[1.0, 1, 0], [1, 1, 1], [1, -1, 0], [-1, 1, 1], [0, 1, 1], [1, 0, -1]])


def plane_diagonal(n, seed=0, M=1):
    """Cubes and bricks at the identity or a product of quarter turns against
    normals (1, 1, 0) / sqrt 2 and (1, 1, 1) / sqrt 3 (and their mirror
    images), the centre on the plane, just below or a little deeper: edges and
    faces parallel to the plane's diagonals, 6 or 7 corners with offset
    distance <= 0."""
    rng = np.random.default_rng(seed)
    G, P = n // M, 2
    normals = _DIAGONALS[rng.integers(0, len(_DIAGONALS), (G, P))]
    normals[:, 0] = _DIAGONALS[rng.integers(0, 2, G)]
    normals = normals / np.linalg.norm(normals, axis=2)[:, :, None]
    h = rng.choice([0.125, 0.25, 0.5], (G * M, 1)) * np.ones((1, 3))
    brick = rng.random(G * M) < 0.3
    h[brick] = rng.choice([0.125, 0.25, 0.5], (int(brick.sum()), 3))
    s = np.sqrt(0.5)
    turns = np.array([[1.0, 0, 0, 0], [s, s, 0, 0], [s, 0, s, 0], [s, 0, 0, s], [0, 1.0, 0, 0], [0.5, 0.5, 0.5, 0.5]])
    quat = turns[rng.integers(0, len(turns), G * M)]
    dists = rng.choice([0.0, -1e-3, -0.05, -0.3, 0.05], (G * M, P)) * np.where(rng.random((G * M, P)) < 0.8, 1, 0)
    return _plane_family("plane_diagonal", n, M, rng, normals, np.full(G * M, BOX, np.int32), h, quat, dists)


FLAT_OFFSETS = (0.0, -2.0 ** -40, 2.0 ** -40)


def plane_flat(n=0, seed=0, M=1):
    """A face, an edge or a vertex of an identity box exactly on the plane and
    2^-40 below and above it, on operands that make the outcome exact: the
    face on z = 0 (4 corners, 4, none), the edge on the plane through the
    origin with the normal (0, s, s), s = fl(sqrt 1/2) (2, 2, none), the
    vertex on the one with the normal (s, s, s), s = fl(sqrt 1/3) (1, 1,
    none; M = 1 only).  The same nine rows repeated with the boxes moved
    along x by multiples of PLANE_SLOT (exact: the planes contain x), whatever n
    and seed; 9 environments at M = 1, 6 at M > 1 (the planes of an
    environment are shared, so M bodies of one case and offset per environment)."""
    s2, s3 = float(np.sqrt(0.5)), float(np.sqrt(1.0 / 3.0))
    cases = [((0.0, 0.0, 1.0), (0.25, 0.5, 0.125), (0.0, 0.0, 0.125), 4),
             ((0.0, s2, s2), (0.5, 0.25, 0.25), (0.0, 0.25, 0.25), 2),
             ((s3, s3, s3), (0.25, 0.25, 0.25), (0.25, 0.25, 0.25), 1)]
    if M > 1:
        cases = cases[:2]
    kind, size, c, planes, expect = [], [], [], [], []
    for nrm, h, at, hits in cases:
        for off in FLAT_OFFSETS:
            planes.append([[*nrm, 0.0, 0.0, 0.0]])
            for b in range(M):
                kind.append(BOX)
                size.append(h)
                c.append([at[0] + (b - M // 2) * PLANE_SLOT, at[1], at[2] + off])
                expect.append(hits if off <= 0 else 0)
    N = len(kind)
    return Problem("plane_flat", M, kind, size, _qpos(c, _ident(N)), np.array(planes), expect)


def plane_deep(n, seed=0, M=1):
    """The box centre below the plane, by up to three bounding radii: between
    four and eight vertices below the plane, the offset test decides."""
    rng = np.random.default_rng(seed)
    G, P = n // M, (3 if M == 1 else 2)
    size = rng.uniform(0.1, 0.5, (G * M, 3))
    dists = -rng.uniform(0.0, 3.0, (G * M, P)) * np.linalg.norm(size, axis=1)[:, None]
    return _plane_family("plane_deep", n, M, rng, _random_normals(rng, G, P), np.full(G * M, BOX, np.int32), size,
                         _unit(rng, G * M, 4), dists)


def plane_spheres(n, seed=0, M=1):
    """Spheres of r = 1/8 over z = 0 at gap 0 and -+2^-40 (hit, hit, miss:
    stated), then spheres with random radii against two random planes at a
    gap of 0, +-1e-12, +-1e-3 or random."""
    rng = np.random.default_rng(seed)
    G, P = n // M, 2
    normals = _random_normals(rng, G, P)
    size = np.zeros((G * M, 3))
    size[:, 0] = rng.uniform(0.05, 0.4, G * M)
    gaps = rng.choice([0.0, 1e-12, -1e-12, 1e-3, -1e-3, 0.3, -0.3], (G * M, P))
    pb = _plane_family("plane_spheres", n, M, rng, normals, np.zeros(G * M, np.int32), size, _ident(G * M),
                       gaps + size[:, :1])
    expect = np.full(pb.N, -1)
    k = 3 if pb.G >= 3 else 0                            # (a single environment keeps its random rows)
    for g in range(k):                                   # the first three environments: the exact rows
        pb.planes[g] = [[0.0, 0, 1, 0, 0, 0], [0.0, 0, 1, 0, 0, -8.0]]
        s = slice(g * M, (g + 1) * M)
        pb.size[s] = [0.125, 0, 0]
        pb.qpos[s, 0] = (np.arange(M) - M // 2) * PLANE_SLOT
        pb.qpos[s, 1] = 0
        pb.qpos[s, 2] = 0.125 + FLAT_OFFSETS[g]
        expect[s] = 1 if FLAT_OFFSETS[g] <= 0 else 0
    pb.expect = expect
    return pb


def _pair_problem(name, c1, r1, c2, r2, M, expect=None, planes=None):
    """n pairs of spheres (bodies 2p and 2p + 1 of the flat order) as
    environments of M bodies: M // 2 pairs each, SLOT apart along x about the
    origin, and a lone sphere far off when M is odd.  M = 0: one environment
    on a cubic lattice of spacing SLOT centred on the origin."""
    n = len(c1)
    if M == 0:
        side = int(np.ceil(n ** (1 / 3)))
        k = np.arange(n)
        at = (np.stack([k % side, (k // side) % side, k // (side * side)], 1) - side // 2) * SLOT
        M_, G = 2 * n, 1
        c = np.stack([c1 + at, c2 + at], 1).reshape(2 * n, 3)
        r = np.stack([r1, r2], 1).reshape(2 * n)
        ex = None if expect is None else np.repeat(expect, 2)
    else:
        per = M // 2
        G = n // per
        M_ = M
        c, r = np.zeros((G, M, 3)), np.full((G, M), 0.1)
        ex = None if expect is None else np.zeros((G, M), np.int64)
        for g in range(G):
            for s in range(per):
                p = g * per + s
                at = np.array([(s - per // 2) * SLOT, 0.0, 0.0])
                c[g, 2 * s], c[g, 2 * s + 1] = c1[p] + at, c2[p] + at
                r[g, 2 * s], r[g, 2 * s + 1] = r1[p], r2[p]
                if ex is not None:
                    ex[g, 2 * s:2 * s + 2] = expect[p]
            if M % 2:
                c[g, M - 1] = [0.0, 3 * SLOT, 0.0]
        c, r = c.reshape(G * M, 3), r.reshape(G * M)
        ex = None if ex is None else ex.reshape(-1)
    size = np.zeros((len(c), 3))
    size[:, 0] = r
    planes = np.tile([[[0.0, 0, 1, 0, 0, -50.0]]], (G, 1, 1)) if planes is None else planes
    return Problem(name, M_, np.zeros(len(c), np.int32), size, _qpos(c, _ident(len(c))), planes, ex)


def pairs_random(n, seed=0, M=0):
    """Unequal radii U(0.05, 0.3); centre distance (r1 + r2) U(0.5, 1.5)."""
    rng = np.random.default_rng(seed)
    r1, r2 = rng.uniform(0.05, 0.3, n), rng.uniform(0.05, 0.3, n)
    c1 = rng.uniform(-0.2, 0.2, (n, 3))
    c2 = c1 + _unit(rng, n) * ((r1 + r2) * rng.uniform(0.5, 1.5, n))[:, None]
    return _pair_problem("pairs_random", c1, r1, c2, r2, M)


SQ_MARGIN = {"f64": 1e-9, "f32": 1e-4}     # csrc/rb_device.hpp sq_margin: the d^2 prefilter's relative margin
GRAZE = (0.0, 0.25, -0.25, 0.75, -0.75, 2.0, -2.0, 8.0, -8.0)


def pairs_grazing(n, seed=0, M=0, dtype="f64"):
    """d^2 = R^2 (1 + m sq_margin) for m in GRAZE, R = r1 + r2 with unequal
    radii, in random directions: inside the prefilter's band, where the square
    root decides, and just outside it on both sides; after these, three
    axis-aligned pairs of r = 1/8 at centre distance 1/4 + (0, -2^-40,
    +2^-40) (stated: hit, hit, miss)."""
    rng = np.random.default_rng(seed)
    r1, r2 = rng.uniform(0.05, 0.3, n), rng.uniform(0.05, 0.3, n)
    c1 = rng.uniform(-0.2, 0.2, (n, 3))
    m = np.array(GRAZE)[np.arange(n) % len(GRAZE)]
    c2 = c1 + _unit(rng, n) * ((r1 + r2) * np.sqrt(1 + m * SQ_MARGIN[dtype]))[:, None]
    expect = np.full(n, -1)
    k = min(3, n)
    r1[-k:], r2[-k:], c1[-k:] = 0.125, 0.125, 0.0
    c2[-k:] = 0
    c2[-k:, 0] = 0.25 + np.array(FLAT_OFFSETS[:k])
    expect[-k:] = np.where(np.array(FLAT_OFFSETS[:k]) <= 0, 1, 0)
    pb = _pair_problem("pairs_grazing", c1, r1, c2, r2, M, expect)
    pb.graze = m[:-k]
    return pb


def pairs_coincident(n, seed=0, M=0):
    """Centres equal (frame (1, 0, 0)) in every other pair, 0.05 apart in a
    random direction in the rest; unequal radii."""
    rng = np.random.default_rng(seed)
    r1, r2 = rng.uniform(0.05, 0.3, n), rng.uniform(0.05, 0.3, n)
    c1 = rng.uniform(-0.2, 0.2, (n, 3))
    c2 = c1 + _unit(rng, n) * np.where(np.arange(n) % 2 == 0, 0.0, 0.05)[:, None]
    return _pair_problem("pairs_coincident", c1, r1, c2, r2, M, np.ones(n, np.int64))


# ---- broadphase: one environment, spheres of r 0.1 unless stated
R0 = 0.1
FINE, COARSE = 2 * R0 * 1.001, 4 * R0 * 1.001       # the oracle's cell and the kernels' cell


def _cloud(name, c, r=None, planes=None, max_partners=16, expect=None):
    N = len(c)
    size = np.zeros((N, 3))
    size[:, 0] = R0 if r is None else r
    planes = np.array([[[0.0, 0, 1, 0, 0, -1e4]]]) if planes is None else planes
    return Problem(name, N, np.zeros(N, np.int32), size, _qpos(c, _ident(N)), planes, expect, max_partners)


def cells_lattice(n, seed=0):
    """Centres on integer multiples of both cell sizes, -6 .. +6 cells per
    axis (the axes, the face diagonals and random lattice points; neighbours
    on the finer lattice are 2 r 1.001 apart and do not touch), each with a
    partner in a random direction at 2 r (1 -+ 1e-3): the partner lies in any
    of the neighbouring cells, by a hair, and may touch other lattice bodies."""
    rng = np.random.default_rng(seed)
    pts = []
    for cs in (FINE, COARSE):
        k = np.arange(-6, 7)
        for a in range(3):
            e = np.zeros((13, 3))
            e[:, a] = k
            pts.append(e * cs)
            e = np.zeros((13, 3))
            e[:, a], e[:, (a + 1) % 3] = k, k[::-1]
            pts.append(e * cs)
    pts = np.concatenate(pts)
    pts = pts[np.sort(np.unique(pts.round(9), axis=0, return_index=True)[1])]
    more = max(n // 2 - len(pts), 0)
    extra = rng.integers(-6, 7, (more, 3)) * np.where(rng.random((more, 1)) < 0.5, FINE, COARSE)
    c1 = np.concatenate([pts, extra])
    c1 = c1[np.sort(np.unique(c1.round(9), axis=0, return_index=True)[1])][:n // 2]
    sign = np.where(np.arange(len(c1)) % 2 == 0, -1.0, 1.0)
    c2 = c1 + _unit(rng, len(c1)) * (2 * R0 * (1 + sign * 1e-3))[:, None]
    pb = _cloud("cells_lattice", np.stack([c1, c2], 1).reshape(-1, 3))
    pb.inside = sign < 0                                  # pair p = bodies 2 p, 2 p + 1 touches
    return pb


HALF_VARIANTS = (("ulp", -1), ("ulp", 0), ("ulp", 1), ("cell", -2e-3), ("cell", 2e-3))


def cells_half(n, seed=0, dtype="f64"):
    """Centres whose coordinate on one axis sits within +-1 ulp of the middle
    of a kernel cell (the switch of the 2 x 2 x 2 search's side) with a partner
    2 r (1 - 1e-3) away straight along that axis on either side, and centres
    2e-3 of a cell to either side of the middle whose partner, as far away on
    that side, lies just across the cell's boundary.  Every axis, cells of
    either sign; each pair in a cell block of its own.  The ulp is that of
    dtype."""
    rng = np.random.default_rng(seed)
    c1, c2 = [], []
    p = 0
    while 2 * len(c1) < n:
        a, (what, amount), side = p % 3, HALF_VARIANTS[(p // 3) % 5], (p // 15) % 2
        cell = rng.integers(-4, 4, 3) + 12 * np.array([p % 7 - 3, (p // 7) % 7 - 3, p // 49 - 3])
        c = (cell + rng.uniform(0.2, 0.8, 3)) * COARSE
        mid = (cell[a] + 0.5) * COARSE
        if what == "ulp" and dtype == "f32":
            mid = np.float32(mid)
            c[a] = float(mid + np.float32(amount) * np.spacing(abs(mid)))
        elif what == "ulp":
            c[a] = mid + amount * np.spacing(abs(mid))
        else:
            c[a] = mid + amount * COARSE
            side = amount > 0
        d = np.zeros(3)
        d[a] = (1 if side else -1) * 2 * R0 * (1 - 1e-3)
        c1.append(c)
        c2.append(c + d)
        p += 1
    pb = _cloud("cells_half", np.stack([np.array(c1), np.array(c2)], 1).reshape(-1, 3), expect=np.ones(2 * len(c1)))
    pb.axis = np.arange(len(c1)) % 3
    return pb


def cells_negative(n, seed=0):
    """A packed cloud entirely in x, y, z < 0: a jittered grid of spacing
    0.19 < 2 r, between three planes that face it from the negative side (a
    floor under it, two walls), the lowest layer resting in the floor."""
    rng = np.random.default_rng(seed)
    side = int(round(n ** (1 / 3)))
    nx, ny = side, side
    nz = -(-n // (nx * ny))
    k = np.arange(nx * ny * nz)[:n]
    grid = np.stack([k % nx, (k // nx) % ny, k // (nx * ny)], 1).astype(float)
    c = -0.3 - 0.19 * grid[:, ::-1] + rng.uniform(-0.02, 0.02, (n, 3))
    lo = c.min(0)
    planes = np.array([[[0.0, 0, 1, 0, 0, lo[2] - 0.09], [1.0, 0, 0, lo[0] - 0.09, 0, 0],
                        [0.0, 1, 0, 0, lo[1] - 0.09, 0]]])
    return _cloud("cells_negative", c, planes=planes)


PERIOD_K = {"f64": 14, "f32": 8}
PERIOD_UNITS = {"f64": 6, "f32": 10}


def cells_period(n=0, seed=0, dtype="f64"):
    """Identical small clusters offset by 4 rmax 1.001 2^k along each axis,
    k = 0 .. PERIOD_K: whatever period the layout picks, two clusters share its
    buckets.  A cluster is six units (ten in fp32) on the cell diagonal (3 i, 3 i, 3 i), a
    unit two touching pairs along x inside one cell, placed so that units in
    neighbouring cells stay 6e-4 apart or more; no two units of different
    clusters share a cell (a difference of diagonal cells has three non-zero
    components, one of shifts at most two).  Whatever n and seed: 46 clusters
    of 24 bodies in fp64, 28 of 40 in fp32."""
    shifts = [np.zeros(3)] + [np.eye(3)[a] * COARSE * 2.0 ** k for a in range(3) for k in range(PERIOD_K[dtype] + 1)]
    t = 2 * R0 * (1 - 1e-3)
    unit = np.array([[0.05, 0.05, 0.05], [0.05 + t, 0.05, 0.05], [0.05, 0.25, 0.25], [0.05 + t, 0.25, 0.25]])
    cluster = np.concatenate([unit + 3 * i * COARSE for i in range(-(PERIOD_UNITS[dtype] // 2), (PERIOD_UNITS[dtype] + 1) // 2)])
    c = np.concatenate([cluster + s for s in shifts])
    return _cloud("cells_period", c, expect=np.ones(len(c)))


def radius_mix(n, seed=0):
    """Spheres of r = 1.0, each ringed by r = 0.05 ones: on its surface
    (touching it, some touching each other) and hovering 0.02 off it.  rmax =
    1 sets the cell size, so a cell holds dozens of bodies that do not touch;
    max_partners 32."""
    rng = np.random.default_rng(seed)
    per = 60
    big = max(1, n // (per + 1))
    c, r = [], []
    for b in range(big):
        centre = np.array([(b % 3 - 1) * 3.0, ((b // 3) % 3 - 1) * 3.0, (b // 9 - 0.5) * 3.0]) + rng.uniform(-.3, .3, 3)
        c.append(centre)
        r.append(1.0)
        u = _unit(rng, per)
        k = 0
        kept = []
        for d in u:                                       # at most 24 small ones touch a big one
            hover = k >= 24
            p = centre + d * (1.0 + 0.05 + (0.02 if hover else -0.002))
            kept.append(p)
            k += 1
        c.extend(kept)
        r.extend([0.05] * per)
    return _cloud("radius_mix", np.array(c), r=np.array(r), max_partners=32)


# ---- the tile form's broadphase: the same edges, thin in z, so that a tile of
# x, y columns holds at most 112 bodies and the form commits (tests/tile_fit.py)
SHEET_TC = (4, 5, 6, 7, 8)


def sheet_lattice(n, seed=0):
    """cells_lattice in a sheet: centres (z = 0) on integer multiples of the
    column COARSE in x and y, first those on multiples of tc COARSE for every
    tile width tc = 4 .. 8 at -3 .. +3 tiles about the origin (corners of
    tiles, on column, tile and slot-row boundaries at once), then random
    columns within +-24; each with a partner at 2 r (1 -+ 1e-3) in a random,
    mostly horizontal direction: across a boundary by a hair, or not."""
    rng = np.random.default_rng(seed)
    k = np.arange(-3, 4)
    pts = [np.stack(np.meshgrid(k * tc, k * tc), -1).reshape(-1, 2) for tc in SHEET_TC]
    pts.append(rng.integers(-24, 25, (n, 2)))
    c1 = np.concatenate(pts)
    c1 = c1[np.sort(np.unique(c1, axis=0, return_index=True)[1])][:n // 2]
    c1 = np.concatenate([c1 * COARSE, np.zeros((len(c1), 1))], 1)
    sign = np.where(np.arange(len(c1)) % 2 == 0, -1.0, 1.0)
    d = rng.normal(size=(len(c1), 3)) * [1.0, 1.0, 0.2]
    d /= np.linalg.norm(d, axis=1)[:, None]
    c2 = c1 + d * (2 * R0 * (1 + sign * 1e-3))[:, None]
    pb = _cloud("sheet_lattice", np.stack([c1, c2], 1).reshape(-1, 3))
    pb.inside = sign < 0
    return pb


def sheet_negative(n, seed=0):
    """cells_negative as a sheet, twice: one layer on a jittered grid of
    spacing 0.19 < 2 r with a sparse second layer resting on it (one sphere
    over every fifth), once entirely in x, y < 0 and once straddling the
    origin (tiles (-1, -1), (0, -1), (-1, 0) and (0, 0) populated), over a
    floor and between two walls that face the cloud from the negative side,
    the lowest bodies resting in them.  Both copies stay within 4 m of the
    origin (13 x 13 and 34 bodies each at n = 406), where the fp32 residuals of
    plane records stay under those measured on cells_negative."""
    rng = np.random.default_rng(seed)
    side = int(np.sqrt(n / 2 / 1.2))
    k = np.arange(side * side)
    base = np.stack([k % side, k // side, np.zeros(len(k))], 1) * [0.19, 0.19, 0.0]
    c = []
    for origin in (np.array([-3.8, -3.8, 0.0]), np.array([-0.19 * (side - 1) / 2, -0.19 * (side - 1) / 2, 0.0])):
        low = origin + base + rng.uniform(-0.02, 0.02, base.shape)
        top = low[::5] + rng.uniform(-0.03, 0.03, (len(low[::5]), 3)) + [0.0, 0.0, 0.185]
        c += [low, top]
    c = np.concatenate(c)[:n]
    lo = c.min(0)
    planes = np.array([[[0.0, 0, 1, 0, 0, lo[2] - 0.09], [1.0, 0, 0, lo[0] - 0.09, 0, 0],
                        [0.0, 1, 0, 0, lo[1] - 0.09, 0]]])
    return _cloud("sheet_negative", c, planes=planes)


def sheet_period(n=0, seed=0, dtype="f64"):
    """cells_period along x and y only: the clusters offset by COARSE 2^k,
    k = 0 .. PERIOD_K, along x, along y and along the antidiagonal (2^k,
    -2^k), a cluster's units on the diagonal columns (3 i, 3 i).  Whatever
    ntx x nty the fold picks, populated tiles share a slot.  No two units of
    different clusters share a column (a difference of two shifts is never a
    multiple of (3, 3) but 0).  31 + 14 clusters of 24 bodies in fp64, 19 + 8
    of 40 in fp32 (the antidiagonal stops at k = PERIOD_K - 1, which keeps
    fp32 within 108 m); every body has one record."""
    K = PERIOD_K[dtype]
    shifts = [np.zeros(3)] + [np.array(a) * COARSE * 2.0 ** k for a in ((1.0, 0, 0), (0, 1.0, 0)) for k in range(K + 1)]
    shifts += [np.array([1.0, -1.0, 0]) * COARSE * 2.0 ** k for k in range(K)]     # (k < K: the units reach 5 m further down)
    t = 2 * R0 * (1 - 1e-3)
    unit = np.array([[0.05, 0.05, 0.05], [0.05 + t, 0.05, 0.05], [0.05, 0.25, 0.25], [0.05 + t, 0.25, 0.25]])
    U = PERIOD_UNITS[dtype]
    cluster = np.concatenate([unit + 3 * i * COARSE * np.array([1.0, 1.0, 0.0]) for i in range(-(U // 2), (U + 1) // 2)])
    c = np.concatenate([cluster + s for s in shifts])
    return _cloud("sheet_period", c, expect=np.ones(len(c)))


SHEET_BIG = 4 * 4 * 1.001       # a tile of width 4 of the 4-m column that r = 1 sets


def sheet_radius(n, seed=0):
    """radius_mix with the r = 1 spheres a tile of four 4-m columns apart (a
    5-wide grid about the origin), each with 24 satellites of r = 0.05
    touching it and 36 hovering 0.02 off it: 61 bodies and 24 partners of one
    body inside one tile; max_partners 32."""
    rng = np.random.default_rng(seed)
    per = 60
    big = max(1, n // (per + 1))
    c, r = [], []
    for b in range(big):
        centre = np.array([(b % 5 - 1.5) * SHEET_BIG, (b // 5 - 1.5) * SHEET_BIG, 0.0]) + rng.uniform(-.3, .3, 3)
        c.append(centre)
        r.append(1.0)
        for k, d in enumerate(_unit(rng, per)):
            c.append(centre + d * (1.0 + 0.05 + (0.02 if k >= 24 else -0.002)))
        r.extend([0.05] * per)
    return _cloud("sheet_radius", np.array(c), r=np.array(r), max_partners=32)


def sheet_piles(n=0, seed=0):
    """tile_fit.piles: vertical stacks of 7 to 20 spheres in one column,
    neighbours 2 r (1 - 1e-3) apart, the lowest 1e-3 r deep in the floor
    z = 0; a few stacks per tile of width 4, some columns with two."""
    import tile_fit
    c, expect = tile_fit.piles(seed=seed)
    return _cloud("sheet_piles", c, planes=np.array([[[0.0, 0, 1, 0, 0, 0.0]]]), expect=expect)


PLANE_FAMILIES = {"plane_random": plane_random, "plane_diagonal": plane_diagonal, "plane_flat": plane_flat,
                  "plane_deep": plane_deep, "plane_spheres": plane_spheres}
PAIR_FAMILIES = {"pairs_random": pairs_random, "pairs_grazing": pairs_grazing, "pairs_coincident": pairs_coincident}
CELL_FAMILIES = {"cells_lattice": cells_lattice, "cells_half": cells_half, "cells_negative": cells_negative,
                 "cells_period": cells_period, "radius_mix": radius_mix}
TILE_FAMILIES = {"sheet_lattice": sheet_lattice, "sheet_negative": sheet_negative, "sheet_period": sheet_period,
                 "sheet_radius": sheet_radius, "sheet_piles": sheet_piles}
FAMILIES = {**PLANE_FAMILIES, **PAIR_FAMILIES, **CELL_FAMILIES, **TILE_FAMILIES}
RANDOM_FAMILIES = ("plane_random", "plane_deep", "pairs_random", "cells_negative", "radius_mix", "mixed",
                   "sheet_negative", "sheet_radius")
DTYPE_FAMILIES = ("pairs_grazing", "cells_half", "cells_period", "sheet_period")   # built for the precision they run in
_widths = {}


def tile_widths(family, dtype="f64"):
    """The tile widths at which the family at CASES holds, by tests/tile_fit.py's
    mirror of the fit: forced to tc the fit keeps tc (the 112 rule does not
    lower it), no slot holds more than 112 bodies and no window more than 384
    records.  Nothing is listed by hand: the GPU tests run every width named
    here, and tests/test_oracle_contact_geometry.py states which ones each
    family must at least reach."""
    import tile_fit
    if (family, dtype) not in _widths:
        pb = make(family, dtype=dtype)
        fits = {tc: tile_fit.fit(pb.qpos, column_size(pb), force=tc) for tc in SHEET_TC}
        _widths[family, dtype] = tuple(tc for tc in SHEET_TC if fits[tc].tc == tc and tile_fit.holds(fits[tc]))
    return _widths[family, dtype]

# family -> (n, seed) of the CPU tests and of the fp32 measurement
CASES = {"plane_random": (2000, 0), "plane_diagonal": (2000, 201), "plane_flat": (9, 202), "plane_deep": (1000, 203),
         "plane_spheres": (1000, 204), "pairs_random": (1000, 205), "pairs_grazing": (903, 206),
         "pairs_coincident": (500, 207), "cells_lattice": (1100, 208), "cells_half": (1100, 209),
         "cells_negative": (1100, 210), "cells_period": (1104, 211), "radius_mix": (1098, 212),
         "sheet_lattice": (1100, 213), "sheet_negative": (406, 214), "sheet_period": (1080, 215),
         "sheet_radius": (1098, 216), "sheet_piles": (0, 217)}


def column_size(pb):
    """The column of a world of the problem's bodies (the hashed cell): 4 rmax 1.001."""
    return 4.0 * float(pb.size[:, 0].max()) * 1.001


def make(family, n=None, seed=None, dtype="f64", **kw):
    """The family's Problem at (n, seed) (default: CASES), built for dtype and
    rounded to fp32 when dtype is f32."""
    n0, s0 = CASES[family]
    if family in DTYPE_FAMILIES:
        kw["dtype"] = dtype
    pb = FAMILIES[family](n0 if n is None else n, s0 if seed is None else seed, **kw)
    return pb.rounded() if dtype == "f32" else pb


def mixed(G, seed=0, M=5):
    """Environments of M bodies in a mix: slot kinds box, sphere, sphere, box,
    sphere, ... (the same in every environment), two random planes; the boxes
    and the odd spheres lie about the planes PLANE_SLOT apart as in plane_random,
    and each sphere that follows a sphere touches or grazes it (a pair), a
    sphere that follows a box lies within the box's bounding sphere."""
    rng = np.random.default_rng(seed)
    pattern = np.array([BOX, SPHERE, SPHERE, BOX, SPHERE, SPHERE, SPHERE], np.int32)
    kind = np.tile(np.resize(pattern, M), G)
    size = rng.uniform(0.1, 0.4, (G * M, 3))
    size[kind == SPHERE, 1:] = 0
    dists = rng.uniform(-1.2, 1.2, (G * M, 2)) * _reach(size, kind == BOX)[:, None]
    pb = _plane_family("mixed", G * M, M, rng, _random_normals(rng, G, 2), kind, size, _unit(rng, G * M, 4), dists)
    for g in range(G):
        for b in range(1, M):
            i = g * M + b
            if kind[i] == SPHERE and b % 7 in (1, 2, 5):
                reach = _reach(pb.size[i - 1:i + 1], kind[i - 1:i + 1] == BOX).sum()
                pb.qpos[i, :3] = pb.qpos[i - 1, :3] + _unit(rng, 1)[0] * reach * rng.uniform(0.3, 1.2)
    return pb
