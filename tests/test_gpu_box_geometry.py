"""The device's box narrowphase (csrc/rb_boxes.hpp through rb_kat_narrow and
through a World's box kernel) on the degenerate input families of
tests/box_geometry.py: bit for bit against the oracle, and, so that the
kernel is judged against the geometry and not only against its twin, held to
the properties of DESIGN §2.5 against the long-double reference, in fp64 at
tol 1e-12 and in fp32 at the measured fp32 bound."""
import numpy as np
import pytest

import box_geometry as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rb():
    import rbhip
    rbhip.load()
    return rbhip


@pytest.fixture(scope="module")
def inputs():
    # 1,000 rows per family (`random` 3,000: the 2 % cap of property 7 needs its 100 edge contacts)
    return {f: G.FAMILIES[f](*G.CASES[f]) for f in G.FAMILIES}


@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_device_equals_oracle_bit_for_bit(rb, oracle, inputs, family):
    inp = inputs[family]
    out, ref = rb.kat_narrow(inp), oracle.kat_narrow(inp)
    bad = np.nonzero((out.view(np.uint64) != ref.view(np.uint64)).any(1))[0]
    assert bad.size == 0, f"fp64: {bad.size} rows differ, first {bad[:5]}: {out[bad[:1]]} vs {ref[bad[:1]]}"
    out, ref = rb.kat_narrow(inp, dtype="f32"), oracle.kat_narrow(inp, dtype="f32")
    bad = np.nonzero((out != ref).any(1))[0]
    assert np.array_equal(out, ref), f"fp32: {bad.size} rows differ, first {bad[:5]}: {out[bad[:1]]} vs {ref[bad[:1]]}"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_device_narrowphase_is_the_geometry(rb, inputs, family, dtype):
    def narrow(x):
        return rb.kat_narrow(x, dtype=dtype)
    inp = inputs[family]
    G.assert_properties(inp, narrow(inp), family, dtype, narrow=narrow)


def test_world_records_are_the_narrowphase(rb):
    """600 pairs from all families on a lattice in one World: one step's
    recorded contacts of both bodies of every pair equal rb.kat_narrow of the
    same operands — the degenerate operands through the deferred queue, the
    orientation snapshot and the box kernel instead of the KAT entry."""
    rows = G.lattice_rows(600)
    mixed = rows[rows[:, 0] != rows[:, 1]]
    assert len(mixed) >= 40 and abs(int((mixed[:, 0] == G.BOX).sum()) * 2 - len(mixed)) <= 1
    expect = rb.kat_narrow(rows)
    with rb.World(G.pair_scene(rows), max_partners=32) as w:
        w.record_contacts(True)
        w.step(1)
        records = w.contacts()
    assert set(records[2].tolist()) == set(G.KINDS)
    G.assert_records_are_the_narrowphase(records, expect)
