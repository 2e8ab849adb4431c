"""The CPU oracle's contact lists (oracle.contacts: rb_oracle_impl.h
plane_sphere, plane_box, sphere_sphere and gen_contacts) held to the
long-double all-pairs reference of tests/contact_geometry.py, in fp64 and on
the fp32 restatement, for every family at contact_geometry.CASES; and the
families held to what they claim to contain.

check_family() is the whole check of one family, so a mutant of the oracle
built apart from the tree can be put through the same code.  Four were, in
fp64 and fp32 alike (none is committed); each row names what failed:

  mutant                               families failing, by property
  plane_box without `ldist > 0`        plane_random (1,932 of 2,000 bodies),
                                       plane_diagonal (355), plane_deep (987)
                                       (3: a listed corner clearly fails the
                                       offset test)
  plane_sphere pos with s = -dist/2+r  plane_spheres, cells_negative (2: pos -
                                       frame dist / 2 is 2 r off the plane: 0.80
                                       and 0.20)
  neighbour loop dz = 0 .. 1 only      pairs_random (85 records missing),
                                       pairs_grazing (26), pairs_coincident
                                       (13), cells_lattice (245), cells_half
                                       (126), cells_negative (725), radius_mix
                                       (136) (4: an overlapping pair is not
                                       listed / is listed on one body only);
                                       not cells_period, whose pairs lie along x
  floor replaced by a cast             none, rightly: truncation makes cell 0
                                       two cells wide on each axis and leaves
                                       every other cell in place, so the 27
                                       cells still cover a body's reach.  An
                                       equivalent mutant of the oracle's
                                       search, not a defect
"""
import numpy as np
import pytest

import contact_geometry as cg
import tile_fit

FAMILY_IDS = list(cg.FAMILIES)


def _cells(pb, cs):
    return np.floor(pb.qpos[:, :3] / cs).astype(np.int64)


def family_claims(pb, lists, rep, dtype):
    """What the family is for, as a list of the claims that do not hold."""
    f, c, cnt, bad = pb.name, rep.counts, lists[0], []
    owner = np.repeat(np.arange(pb.N), cnt)
    partners = np.bincount(owner[lists[1] >= 0], minlength=pb.N)
    limit = 32 if f in ("radius_mix", "sheet_radius") else 12
    if partners.max() > limit:
        bad.append(f"a body has {partners.max()} partners (at most {limit})")
    if f == "plane_random" and not (pb.P == cg.MAX_PLANES and c["corner_records"] > 2 * pb.N
                                    and set(range(1, 9)) <= set(lists[2].tolist())):
        bad.append(f"plane_random: {pb.P} planes, {c['corner_records']} corner records")
    if f == "plane_diagonal" and not c["many_corner_rows"] > 0.25 * c["box_plane_rows"]:
        bad.append(f"plane_diagonal: {c['many_corner_rows']} of {c['box_plane_rows']} rows have more than 4 passing corners")
    if f == "plane_deep" and c["corner_records"] != 4 * c["box_plane_rows"]:
        bad.append(f"plane_deep: {c['corner_records']} corners on {c['box_plane_rows']} rows, 4 each follow from a centre below the plane")
    if f == "plane_flat" and c["near_bodies"] != pb.N:
        bad.append("plane_flat: a body is not within near of a plane")
    if f == "plane_spheres" and not (c["near_bodies"] > 0.4 * pb.N and (pb.expect >= 0).sum() == 3 * pb.M):
        bad.append(f"plane_spheres: {c['near_bodies']} near bodies")
    if f == "pairs_random" and not 0.3 * pb.N < 2 * c["sphere_pairs"] < 0.7 * pb.N:
        bad.append(f"pairs_random: {c['sphere_pairs']} touching pairs of {pb.N // 2}")
    if f == "pairs_grazing":
        m = pb.graze
        hit = cnt[0:2 * len(m):2] > 0
        for lo, hi, want in ((-9, -1, True), (1, 9, False)):         # outside the prefilter's band: decided on d^2
            sel = (m > lo) & (m < hi)
            if not (sel.sum() >= 150 and (hit[sel] == want).all()):
                bad.append(f"pairs_grazing: {int(sel.sum())} pairs at m in ({lo}, {hi}), {int(hit[sel].sum())} of them hit")
        for lo, hi in ((-1, 0), (0, 1)):                             # inside it: the square root decides
            sel = (m > lo) & (m < hi)
            if sel.sum() < 150:
                bad.append(f"pairs_grazing: {int(sel.sum())} pairs at m in ({lo}, {hi})")
        if dtype == "f64" and not (hit[(m > -1) & (m < 0)].all() and not hit[(m > 0) & (m < 1)].any()):
            bad.append("pairs_grazing: a pair inside the band is decided against the sign of m")
    if f == "pairs_coincident" and not (c["coincident_records"] == pb.N // 2 and c["ss_records"] == pb.N):
        bad.append(f"pairs_coincident: {c['coincident_records']} records with equal centres")
    if f == "cells_lattice":
        on = [np.abs(pb.qpos[0::2, :3] / cs - np.round(pb.qpos[0::2, :3] / cs)).max(1) < 1e-6 for cs in (cg.FINE, cg.COARSE)]
        span = np.abs(np.round(pb.qpos[0::2, :3] / cg.COARSE)).max()
        if not ((on[0] | on[1]).all() and on[0].sum() > 100 and on[1].sum() > 100 and span == 6):
            bad.append("cells_lattice: centres off the lattices")
        first = np.concatenate([[0], np.cumsum(cnt)])[:-1]
        listed = np.array([(2 * p + 1) in lists[1][first[2 * p]:first[2 * p] + cnt[2 * p]] for p in range(pb.N // 2)])
        if not (listed == pb.inside).all():
            bad.append(f"cells_lattice: {int((listed != pb.inside).sum())} partners at 2 r (1 -+ 1e-3) decided wrongly")
    if f == "cells_half":
        frac = pb.qpos[0::2, :3] / cg.COARSE
        frac = (frac - np.floor(frac))[np.arange(pb.N // 2), pb.axis]
        across = (_cells(pb, cg.COARSE)[0::2] != _cells(pb, cg.COARSE)[1::2]).any(1)
        at = 1e-6 if dtype == "f64" else 2e-5              # 1 ulp of a coordinate of 50 is 1e-5 cells in fp32
        if not ((np.abs(frac - 0.5) < at).sum() >= 0.5 * len(frac) and across.sum() >= 0.3 * len(frac)
                and (_cells(pb, cg.COARSE) < 0).any(0).all()):
            bad.append(f"cells_half: {(np.abs(frac - 0.5) < at).sum()} centres at the switch, {across.sum()} pairs across a boundary")
    if f == "cells_negative":
        planes_hit = set(lists[1][lists[1] < 0].tolist())
        if not ((pb.qpos[:, :3] < 0).all() and (_cells(pb, cg.COARSE).max(0) < 0).all() and c["sphere_pairs"] > pb.N
                and planes_hit == {-1, -2, -3} and len(np.unique(_cells(pb, cg.COARSE), axis=0)) > 50):
            bad.append(f"cells_negative: {c['sphere_pairs']} pairs, planes {planes_hit}")
    if f == "cells_period":
        cell = _cells(pb, cg.COARSE)
        far = [(cell[:, a] > 2 ** 10).sum() for a in range(3)]
        want = 2 if dtype == "f64" else 0
        if not (all(x >= want * 24 for x in far) and c["sphere_pairs"] == pb.N // 2):
            bad.append(f"cells_period: bodies past 2^10 cells per axis {far}, {c['sphere_pairs']} pairs")
    if f == "radius_mix":
        _, per_cell = np.unique(_cells(pb, 4 * 1.001), axis=0, return_counts=True)
        if not (per_cell.max() > 30 and partners.max() >= 20 and pb.max_partners == 32
                and len(np.unique(pb.size[:, 0])) == 2):
            bad.append(f"radius_mix: {per_cell.max()} bodies in the fullest cell, {partners.max()} partners at most")
    if f in cg.TILE_FAMILIES:
        bad += sheet_claims(pb, lists, rep, dtype, partners)
    return bad


def sheet_claims(pb, lists, rep, dtype, partners):
    """The tile-shaped families: what tests/tile_fit.py's mirror of the fit
    says the tile form will meet, at every width the family is run at."""
    f, c, cnt, bad = pb.name, rep.counts, lists[0], []
    col = cg.column_size(pb)
    cols = tile_fit.columns(pb.qpos, col)
    fits = {tc: tile_fit.fit(pb.qpos, col, force=tc) for tc in cg.SHEET_TC}
    # the widths the GPU tests run are the mirror's (cg.tile_widths); stated here so that a change of a
    # family that moves them is seen: all five at 4, the lattice and the period at every width; at the
    # others the 112 rule lowers the forced width (sheet_negative at 5 and 8, sheet_radius from 6 on,
    # sheet_piles from 5 on)
    widths = {"sheet_lattice": cg.SHEET_TC, "sheet_negative": (4, 6, 7), "sheet_period": cg.SHEET_TC,
              "sheet_radius": (4, 5), "sheet_piles": (4,)}[f]
    if cg.tile_widths(f, dtype) != widths:
        bad.append(f"{f}: holds at the widths {cg.tile_widths(f, dtype)}, stated {widths}")
    for tc in cg.SHEET_TC:
        kept = fits[tc].tc == tc and tile_fit.holds(fits[tc])
        if kept != (tc in widths) or (not kept and fits[tc].tc >= tc):
            bad.append(f"{f}: at the forced width {tc}: {fits[tc]}")
    if f == "sheet_lattice":
        k = np.round(pb.qpos[0::2, :2] / cg.COARSE).astype(np.int64)          # the centres' lattice points
        on = np.abs(pb.qpos[0::2, :2] / cg.COARSE - k).max(1) < (1e-9 if dtype == "f64" else 1e-5)   # (9.6 m in fp32: 1e-6 columns)
        first = np.concatenate([[0], np.cumsum(cnt)])[:-1]
        listed = np.array([(2 * p + 1) in lists[1][first[2 * p]:first[2 * p] + cnt[2 * p]] for p in range(pb.N // 2)])
        if not (on.all() and (listed == pb.inside).all()):
            bad.append(f"sheet_lattice: {int((~on).sum())} centres off the lattice, {int((listed != pb.inside).sum())} partners decided wrongly")
        for tc in cg.SHEET_TC:
            t = np.floor_divide(cols, tc)
            corner = (np.mod(k, tc) == 0).all(1).sum()
            ax = [int(((t[0::2, a] != t[1::2, a]) & pb.inside).sum()) for a in range(2)]
            rows = np.mod(t[:, 1], fits[tc].nty)
            if not (corner >= 49 and min(ax) >= 10 and (t < 0).any(0).all() and ((rows[0::2] != rows[1::2]) & pb.inside).sum() >= 10):
                bad.append(f"sheet_lattice, width {tc}: {corner} centres on tile corners, touching pairs across a tile boundary per axis {ax}")
    if f == "sheet_negative":
        tiles = set(map(tuple, np.floor_divide(cols, 4).tolist()))
        half = pb.N // 2
        planes_hit = set(lists[1][lists[1] < 0].tolist())
        if not ({(-1, -1), (0, -1), (-1, 0), (0, 0)} <= tiles and (pb.qpos[:half, :2] < 0).all() and (np.floor_divide(cols[:half], 4) < 0).all()
                and c["sphere_pairs"] > pb.N and planes_hit == {-1, -2, -3} and fits[4].worst_column > tile_fit.WR):
            bad.append(f"sheet_negative: {c['sphere_pairs']} pairs, planes {planes_hit}, tiles about the origin "
                       f"{sorted(t for t in tiles if max(map(abs, t)) <= 1)}")
    if f == "sheet_period":
        far = [(cols[:, a] > 2 ** 10).sum() for a in range(2)] + [(cols[:, 1] < -2 ** 10).sum()]
        want = 2 if dtype == "f64" else 0
        if not (all(x >= want * 24 for x in far) and c["sphere_pairs"] == pb.N // 2 and np.abs(pb.qpos[:, 2]).max() < 0.3):
            bad.append(f"sheet_period: bodies past 2^10 columns {far}, {c['sphere_pairs']} pairs")
        for tc in cg.SHEET_TC:
            if not (fits[tc].folded and fits[tc].aliased >= 2):
                bad.append(f"sheet_period, width {tc}: {fits[tc].aliased} populated tiles share a slot: {fits[tc]}")
    if f == "sheet_radius":
        big = pb.size[:, 0] == 1.0
        tiles = np.floor_divide(cols[big], 4)
        if not (len(np.unique(tiles, axis=0)) == big.sum() and (partners[big] == 24).all() and partners.max() == 24
                and pb.max_partners == 32 and fits[4].worst_column > 12):
            bad.append(f"sheet_radius: {len(np.unique(tiles, axis=0))} tiles for {big.sum()} big spheres, partners {partners[big].tolist()}")
    if f == "sheet_piles":
        ring = fits[4].window_cols.copy()
        ring[:, :, 1:-1, 1:-1] = 0
        per_column = np.unique(cols, axis=0, return_counts=True)[1]
        if not (fits[4].worst_column > 12 and (fits[4].cols > tile_fit.WR).sum() >= 50 and ring.max() > 12
                and 7 <= per_column.min() and (cnt == pb.expect).all()):
            bad.append(f"sheet_piles: the fullest column holds {fits[4].worst_column}, the fullest ring column {ring.max()}")
    return bad


def check_family(oracle, family, dtype):
    pb = cg.make(family, dtype=dtype)
    lists = cg.oracle_lists(oracle, pb, dtype)
    rep = cg.assert_properties(lists, pb, dtype)
    bad = family_claims(pb, lists, rep, dtype)
    assert not bad, "\n".join(bad) + f"\n{rep}"
    return rep


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("family", FAMILY_IDS)
def test_oracle_holds_the_properties(oracle, family, dtype):
    check_family(oracle, family, dtype)


def test_random_families_stay_clear_of_near(oracle):
    """The 1 % cap is a condition the oracle meets with room: the observed
    shares of the module docstring."""
    for family in cg.RANDOM_FAMILIES:
        if family in cg.FAMILIES:
            for dtype in ("f64", "f32"):
                rep = check_family(oracle, family, dtype)
                assert rep.counts["near_bodies"] <= 1, (family, dtype, rep.counts)


def test_fp32_bounds_trace_to_the_measurement(oracle):
    """F32_MEASURED is what the oracle's fp32 restatement gives at CASES; tol is
    8 x its worst residual and near the power of ten above 8 x the largest gap
    of a decision that differed."""
    worst = {}
    for family in cg.FAMILIES:
        pb = cg.make(family, dtype="f32")
        rep = cg.measure(cg.oracle_lists(oracle, pb, "f32"), cg.reference_lists(pb), cg.NEAR["f32"])
        assert not rep.fails, rep.fails
        for k, v in rep.res.items():
            worst[k] = max(worst.get(k, 0.0), v)
    assert set(worst) == set(cg.F32_MEASURED)
    for k, v in worst.items():
        assert v <= cg.F32_MEASURED[k] * 1.005 and v >= cg.F32_MEASURED[k] * 0.995, (k, v, cg.F32_MEASURED[k])
    top = max(v for k, v in cg.F32_MEASURED.items() if k != "decision")
    assert 8 * top <= cg.TOL["f32"] <= 8.1 * top
    assert cg.NEAR["f32"] / 10 < 8 * cg.F32_MEASURED["decision"] <= cg.NEAR["f32"]
    assert max(np.abs(cg.make(f, dtype="f32").qpos[:, :3]).max() for f in cg.FAMILIES) < 108.0


def test_fp64_residuals_stay_below_the_bound(oracle):
    """The oracle's worst fp64 residual over all families, next to tol 1e-12."""
    worst = 0.0
    for family in cg.FAMILIES:
        pb = cg.make(family)
        rep = cg.measure(cg.oracle_lists(oracle, pb), cg.reference_lists(pb), cg.NEAR["f64"])
        worst = max([worst] + [v for k, v in rep.res.items() if k != "decision"])
    assert worst < 5e-13, worst


@pytest.mark.parametrize("M", [5, 14])
def test_mixed_environments(oracle, M):
    """The mixed environments of the batch tests: planes, sphere pairs and
    sphere-box partners in one list, in the stated order."""
    pb = cg.mixed(40, seed=300 + M, M=M)
    lists = cg.oracle_lists(oracle, pb)
    rep = cg.assert_properties(lists, pb)
    c = rep.counts
    assert c["corner_records"] > 40 and c["ss_records"] > 20 and c["box_pair_records"] > 10, c


def test_the_properties_reject_wrong_lists(oracle):
    """A list with one corner dropped, a pair's record removed from one body,
    a normal flipped or two records exchanged does not pass."""
    pb = cg.make("plane_diagonal", n=200)
    good = cg.oracle_lists(oracle, pb)
    ref = cg.reference_lists(pb)
    assert not cg.measure(good, ref, 1e-9).fails

    def drop(lists, k):
        cnt = lists[0].copy()
        cnt[np.searchsorted(np.cumsum(lists[0]), k, side="right")] -= 1
        return (cnt,) + tuple(np.delete(a, k, axis=0) for a in lists[1:])
    many = np.nonzero(good[0] >= 4)[0][0]
    first = int(np.cumsum(good[0])[many] - good[0][many])
    assert any(t.startswith("3:") for t in cg.measure(drop(good, first), ref, 1e-9).fails)
    swapped = tuple(a.copy() for a in good)
    for a in swapped[1:]:
        a[[first, first + 1]] = a[[first + 1, first]]
    assert any(t.startswith("1:") for t in cg.measure(swapped, ref, 1e-9).fails)
    flipped = tuple(a.copy() for a in good)
    flipped[5][first] *= -1
    assert cg.measure(flipped, ref, 1e-9).failures(1e-12)
    pb = cg.make("pairs_random", n=100)
    good = cg.oracle_lists(oracle, pb)
    ref = cg.reference_lists(pb)
    k = int(np.nonzero(good[1] >= 0)[0][0])
    assert any(t.startswith("4:") for t in cg.measure(drop(good, k), ref, 1e-9).fails)
