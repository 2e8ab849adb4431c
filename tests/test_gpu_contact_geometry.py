"""The device's contact lists held to the long-double all-pairs reference of
tests/contact_geometry.py, and compared word for word with the
oracle as the other device tests do.  Every case does both: the first shows
that the kernel's own output is geometrically right at states the committed
trajectories never reach, the second that the anchor and the bit-exact suite
speak about the same lists.

Batch query (BatchWorld.from_scenes, set_planes, set_state, then contacts()
with no step in between: the state is exactly the family's): every plane and
pair family as environments of M = 1 or 2, 14 and 64 bodies and the mixed
environments of M = 5, with E never a multiple of the environments per wave;
fp64 and fp32 batches; the device form with float32 outputs once.

World (set_state, record_contacts, step(1), contacts(): the records are those
of the step-start state; they carry no pos / frame): the broadphase families
through the six step forms of test_gpu_parity.py's
test_ragged_scene_every_step_form_bit_exact, the form asserted from the
stats, in fp64 and through two forms in fp32; the plane families, boxes and
spheres PLANE_SLOT apart along the planes' common direction, through the helper
forms (whose helper wave solves the box corners) and the plain ones.

Tile form (RBHIP_TILE=1; two steps, as a run of one step is never tiled; a
state at rest is unchanged by the first): cells_half is committed without a
roll-back.  The form declines the other four: cells_lattice, cells_negative,
cells_period and radius_mix pack more bodies over one tile of x, y columns
than a slot steps (they are three-dimensional clouds; the run raises
TILE_WHY_CAP), the run is rolled back and the world steps hashed; that their
records are right all the same is asserted too.  Their edges reach the tile
broadphase through contact_geometry.TILE_FAMILIES, thin in z: each is
committed at every tile width at which tests/tile_fit.py's mirror of the fit
says it holds (RBHIP_TILE_COLS; sheet_lattice and sheet_period at 4 .. 8), in
fp64 and at one width in fp32, with the form, the steps, the width and the
slot count asserted from the stats."""
import numpy as np
import pytest

import contact_geometry as cg

pytestmark = pytest.mark.gpu

# hashed_form of rb_world_stats, and the switches of tests/test_gpu_parity.py
FORMS = {
    "coop": (1, {"RBHIP_HELP_MAX_BODIES": "0"}),
    "coop_help": (3, {"RBHIP_HELP_MAX_BODIES": "100000"}),
    "wide": (4, {"RBHIP_COOP_MAX_BODIES": "0"}),
    "wide_plain": (2, {"RBHIP_COOP_MAX_BODIES": "0", "RBHIP_WIDE_HELP": "0"}),
    "one": (0, {"RBHIP_COOP_MAX_BODIES": "0", "RBHIP_WIDE_MAX_BODIES": "0"}),
    "split": (0, {"RBHIP_COOP_MAX_BODIES": "0", "RBHIP_WIDE_MAX_BODIES": "0", "RBHIP_SPLIT": "1"}),
}
SWITCHES = ("RBHIP_COOP_MAX_BODIES", "RBHIP_WIDE_MAX_BODIES", "RBHIP_HELP_MAX_BODIES", "RBHIP_WIDE_HELP", "RBHIP_SPLIT",
            "RBHIP_TABLE_EPOCH", "RBHIP_TILE")


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


def _setenv(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


_cache = {}


def _case(oracle, key, build, dtype):
    """A problem, its reference and the oracle's lists: computed once, shared,
    never modified."""
    if key not in _cache:
        pb = build()
        lists = cg.oracle_lists(oracle, pb, dtype)
        for a in lists + (pb.qpos, pb.size, pb.planes):
            a.setflags(write=False)
        _cache[key] = (pb, cg.reference_lists(pb), lists)
    return _cache[key]


def _same(got, want, dtype):
    """Word for word in fp64; the same values in fp32 (both sides hold floats
    widened to double)."""
    bad = []
    for name, g, w in zip(("counts", "partner", "kind", "dist", "pos", "frame"), got, want):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if g.shape != w.shape:
            bad.append(name)
        elif g.dtype.kind == "f" and dtype == "f64":
            if not np.array_equal(g.view(np.uint64), w.view(np.uint64)):
                bad.append(name)
        elif not np.array_equal(g, w):
            bad.append(name)
    return bad


# ------------------------------------------------------------ the batch query
# family, M, E: E is no multiple of the 64 // M environments of a wave (M = 64: one per wave).
# The bodies of a plane family's environment lie up to M m from the point both
# planes pass through, and the rounding of (c - pp).n grows with that distance:
# 64 m x 2^-24 is 4e-6, above the fp32 near, which was measured within 3 m.  So
# the plane families run at M = 64 in fp64 only; a pair's gap is a difference
# of neighbouring coordinates and keeps its accuracy out there.
BATCH = [(f, M, E) for f in cg.PLANE_FAMILIES for M, E in ((1, 333), (14, 37), (64, 5))] + \
        [(f, M, E) for f in cg.PAIR_FAMILIES for M, E in ((2, 45), (14, 37), (64, 5))] + [("mixed", 5, 27)]
BATCH_TYPED = [(f, M, E, d) for f, M, E in BATCH for d in ("f64", "f32")
               if not (d == "f32" and M == 64 and f in cg.PLANE_FAMILIES)]


def _batch_problem(family, M, E, dtype):
    if family == "mixed":
        pb = cg.mixed(E, seed=300 + M, M=M)
        return pb.rounded() if dtype == "f32" else pb
    n = E * M if family in cg.PLANE_FAMILIES else E * (M // 2)
    return cg.make(family, n=n, dtype=dtype, M=M)


def _query(rb, pb, dtype, device_f32=False):
    scs = pb.scenes()
    with rb.BatchWorld.from_scenes(scs, dtype=dtype) as b:
        b.set_planes(pb.planes)
        b.set_state(pb.qpos.reshape(pb.G, pb.M, 7), np.zeros((pb.G, pb.M, 6)))
        if not device_f32:
            con = b.contacts(max_records=32)
            assert con.truncated == 0
            return cg.dense_lists(con)
        dev = b.contacts_device(max_records=32, dtype="f32")
        assert b.sync() == 0
        import torch
        assert dev.dist.dtype == torch.float32 and dev.frame.dtype == torch.float32
        host = rb.BatchContacts(32, *(getattr(dev, f).cpu().numpy() for f in ("counts", "partner", "kind")),
                                *(getattr(dev, f).cpu().numpy().astype(np.float64) for f in ("dist", "pos", "frame")), None)
        return cg.dense_lists(host)


@pytest.mark.parametrize("family,M,E,dtype", BATCH_TYPED, ids=[f"{f}-M{M}-{d}" for f, M, E, d in BATCH_TYPED])
def test_batch_query(rb, oracle, family, M, E, dtype):
    pb, ref, want = _case(oracle, ("batch", family, M, dtype), lambda: _batch_problem(family, M, E, dtype), dtype)
    assert pb.M == M and (M == 64 or pb.G % (64 // M) != 0) and want[0].sum() > 0 and want[0].max() <= 32
    got = _query(rb, pb, dtype)
    cg.assert_properties(got, pb, dtype, ref)
    assert not _same(got, want, dtype)


@pytest.mark.parametrize("family,M,E", [("plane_random", 1, 333), ("plane_diagonal", 14, 37), ("pairs_random", 64, 5),
                                        ("mixed", 5, 27)], ids=lambda v: str(v))
def test_batch_device_form_float32_outputs(rb, oracle, family, M, E):
    """An fp64 batch's lists written as float32 by the device form: the fp64
    problem's properties at the fp32 bounds, and the oracle's values rounded."""
    pb, ref, want = _case(oracle, ("batch", family, M, "f64"), lambda: _batch_problem(family, M, E, "f64"), "f64")
    got = _query(rb, pb, "f64", device_f32=True)
    cg.assert_properties(got, pb, "f32", ref)
    rounded = want[:3] + tuple(a.astype(np.float32).astype(np.float64) for a in want[3:])
    assert not _same(got, rounded, "f32")


# ------------------------------------------------------------ a World, every step form
def _world_lists(rb, pb, dtype, steps=1):
    sc = pb.scene(0)
    with rb.World(sc, dtype=dtype, max_partners=pb.max_partners) as w:
        w.set_state(pb.qpos, np.zeros((pb.N, 6)))
        w.record_contacts(True)
        w.step(steps)
        return w.contacts(), w.stats()


def _check_world(pb, ref, want, got, dtype):
    cg.assert_properties(got, pb, dtype, ref)
    assert not _same(got, want[:4], dtype)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("family", list(cg.CELL_FAMILIES))
def test_world_broadphase_every_step_form(rb, oracle, monkeypatch, family, form):
    code, env = FORMS[form]
    _setenv(monkeypatch, env)
    pb, ref, want = _case(oracle, ("world", family, "f64"), lambda: cg.make(family), "f64")
    assert pb.G == 1 and 1000 <= pb.N <= 1200 and pb.N % 64 != 0
    got, st = _world_lists(rb, pb, "f64")
    assert st["hashed_form"] == code and st["form"] == code, st
    _check_world(pb, ref, want, got, "f64")


@pytest.mark.parametrize("form", ["coop_help", "wide"])
@pytest.mark.parametrize("family", list(cg.CELL_FAMILIES))
def test_world_broadphase_f32(rb, oracle, monkeypatch, family, form):
    code, env = FORMS[form]
    _setenv(monkeypatch, env)
    pb, ref, want = _case(oracle, ("world", family, "f32"), lambda: cg.make(family, dtype="f32"), "f32")
    assert pb.G == 1 and 1000 <= pb.N <= 1200 and pb.N % 64 != 0
    got, st = _world_lists(rb, pb, "f32")
    assert st["hashed_form"] == code, st
    _check_world(pb, ref, want, got, "f32")


WORLD_PLANE_N = 1100


@pytest.mark.parametrize("form", ["coop", "coop_help", "wide", "wide_plain"])
@pytest.mark.parametrize("family", ["plane_random", "plane_diagonal", "plane_deep", "plane_spheres"])
def test_world_planes(rb, oracle, monkeypatch, family, form):
    """1,100 bodies of one world on two planes, PLANE_SLOT apart along the direction
    both planes contain: out of each other's reach, so every record is a plane
    record (plane_random mixes spheres and boxes)."""
    code, env = FORMS[form]
    _setenv(monkeypatch, env)
    pb, ref, want = _case(oracle, ("world", family, "f64"),
                          lambda: cg.make(family, n=WORLD_PLANE_N, M=WORLD_PLANE_N), "f64")
    assert pb.G == 1 and pb.N % 64 != 0 and (want[1] < 0).all() and want[0].sum() > pb.N // 2
    got, st = _world_lists(rb, pb, "f64")
    assert st["hashed_form"] == code, st
    _check_world(pb, ref, want, got, "f64")


@pytest.mark.parametrize("form", ["coop_help", "wide"])
def test_world_plane_flat(rb, oracle, monkeypatch, form):
    """A face and an edge exactly on the plane and 2^-40 to either side, 70
    boxes of a world each: the stated counts (4, 4, 0 and 2, 2, 0)."""
    code, env = FORMS[form]
    _setenv(monkeypatch, env)
    whole, _, _ = _case(oracle, ("world", "plane_flat", "f64"), lambda: cg.make("plane_flat", M=70), "f64")
    for g in range(whole.G):
        pb, ref, want = _case(oracle, ("world", "plane_flat", g), lambda: whole.only(g), "f64")
        got, st = _world_lists(rb, pb, "f64")
        assert st["hashed_form"] == code, st
        _check_world(pb, ref, want, got, "f64")


# ------------------------------------------------------------ the tile form
TILE_WHY_CAP = 1


def test_world_tile_form(rb, oracle, monkeypatch):
    _setenv(monkeypatch, {"RBHIP_TILE": "1"})
    pb, ref, want = _case(oracle, ("world", "cells_half", "f64"), lambda: cg.make("cells_half"), "f64")
    got, st = _world_lists(rb, pb, "f64", steps=2)
    assert st["form"] == 5 and st["tile_rollbacks"] == 0 and st["tile_steps"] == 2, st
    _check_world(pb, ref, want, got, "f64")


# every width at which the mirror of the fit says the family holds; in fp32 the middle one of those
TILE_CASES = [(f, tc) for f in cg.TILE_FAMILIES for tc in cg.tile_widths(f)]
TILE_F32_WIDTH = {f: cg.tile_widths(f, "f32")[len(cg.tile_widths(f, "f32")) // 2] for f in cg.TILE_FAMILIES}


def _tile_family(rb, oracle, monkeypatch, family, tc, dtype):
    """A tile-shaped family (contact_geometry.TILE_FAMILIES) committed by the
    tile form at the forced width tc: the grid is the one tests/tile_fit.py's
    mirror of the fit gives, both steps ran in tile slots, and the records are
    right by the reference and equal to the oracle's."""
    import tile_fit
    _setenv(monkeypatch, {"RBHIP_TILE": "1", "RBHIP_TILE_COLS": str(tc)})     # (read at the fit: set until the steps ran)
    pb, ref, want = _case(oracle, ("world", family, dtype), lambda: cg.make(family, dtype=dtype), dtype)
    fit = tile_fit.fit(pb.qpos, cg.column_size(pb), force=tc)
    assert fit.tc == tc and tile_fit.holds(fit), fit
    got, st = _world_lists(rb, pb, dtype, steps=2)
    monkeypatch.delenv("RBHIP_TILE_COLS")
    assert st["form"] == 5 and st["tile_rollbacks"] == 0 and st["tile_steps"] == 2 and st["tile_why"] == 0, st
    assert st["tile_cols"] == tc and st["tile_slots"] == fit.slots, (st, fit)
    _check_world(pb, ref, want, got, dtype)


@pytest.mark.parametrize("family,tc", TILE_CASES, ids=[f"{f}-tc{tc}" for f, tc in TILE_CASES])
def test_world_tile_family(rb, oracle, monkeypatch, family, tc):
    _tile_family(rb, oracle, monkeypatch, family, tc, "f64")


@pytest.mark.parametrize("family", list(cg.TILE_FAMILIES))
def test_world_tile_family_f32(rb, oracle, monkeypatch, family):
    _tile_family(rb, oracle, monkeypatch, family, TILE_F32_WIDTH[family], "f32")


@pytest.mark.parametrize("family", ["cells_lattice", "cells_negative", "cells_period", "radius_mix"])
def test_world_tile_form_declined(rb, oracle, monkeypatch, family):
    _setenv(monkeypatch, {"RBHIP_TILE": "1"})
    pb, ref, want = _case(oracle, ("world", family, "f64"), lambda: cg.make(family), "f64")
    got, st = _world_lists(rb, pb, "f64", steps=2)
    assert st["tile_rollbacks"] == 1 and st["tile_steps"] == 0 and st["tile_why"] == TILE_WHY_CAP, st
    _check_world(pb, ref, want, got, "f64")
