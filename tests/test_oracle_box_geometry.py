"""The oracle's box narrowphase (rb_oracle_impl.h "box pairs") against the
long-double geometric reference of tests/box_geometry.py, on CPU: every
property of DESIGN §2.5 on every input family, 1,000 rows each (`random`
3,000), in fp64 at tol 1e-12 and on the fp32 restatement at the measured fp32
bound (box_geometry.F32_MEASURED).  The device is held to the same properties
in tests/test_gpu_box_geometry.py."""
import numpy as np
import pytest

import box_geometry as G


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_oracle_narrowphase_is_the_geometry(oracle, family, dtype):
    rows, seed = G.CASES[family]
    inp = G.FAMILIES[family](rows, seed)

    def narrow(x):
        return oracle.kat_narrow(x, dtype=dtype)
    rep = G.assert_properties(inp, narrow(inp), family, dtype, narrow=narrow)
    if dtype == "f32":
        # the recorded measurement (three digits) is this run's
        got = dict(rep.res, **{k: rep.capped_needed(k) for k in rep.caps})
        over = {k: v for k, v in got.items() if v > 1.01 * G.F32_MEASURED[k]}
        assert not over, f"above box_geometry.F32_MEASURED: {over}"


def test_f32_bound_is_eight_times_the_measurement():
    worst = max(v for k, v in G.F32_MEASURED.items() if k != "decision")
    assert 8 * worst <= G.TOL["f32"] <= 8.1 * worst and G.TOL["f32"] <= 1e-4
    assert 8 * G.F32_MEASURED["decision"] <= G.NEAR["f32"]
    assert G.TOL["f64"] == 1e-12 and G.NEAR["f64"] == 1e-9
    assert (G.SKIP_CAP, G.EDGE_MISS_CAP, G.MISMATCH_CAP) == (0.01, 0.02, 0.005)


def test_random_rows_are_the_recorded_ones():
    """The shared generator keeps the rows tests/test_gpu_boxes.py has always
    drawn (n random pairs and the nine axis-aligned stacks)."""
    a = G.random(50, seed=1)
    assert a.shape == (59, 22) and a[:50, :2].sum() == 47
    assert np.allclose(a[3], [0, 0, 0, 0, 0, 0.428595, 0.643285, 0.231603, -0.590636, 0.1, 0, 0, 0.578054, 0.602459,
                              -0.044944, 0.444578, -0.304693, 0.534209, -0.651256, 0.1, 0, 0], atol=1e-6, rtol=0)
    assert a[:50].sum() == pytest.approx(87.60394874118919, abs=1e-9)
    assert np.array_equal(a[50], [1, 1, 0, 0, 0, 1, 0, 0, 0, .4, .4, .4, 0, .1, .79, 1, 0, 0, 0, .4, .4, .4])


def test_reference_on_hand_cases():
    """The reference itself on cases done by hand: a cube stack's overlap, a
    45-degree edge cross, the surface distance, sphere on and inside a box."""
    one = np.ones((1, 3))
    R = G.rotation([[1, 0, 0, 0]])
    va, vb = G.vertices(0 * one, R, 0.4 * one), G.vertices([[0.5, 0.3, 0.79]], R, 0.4 * one)
    assert float(G.min_overlap(R, R, va, vb)[0]) == pytest.approx(0.01, abs=1e-15)
    assert float(G.overlap(va, vb, np.array([[1.0, 0, 0]], G.LD))[0]) == pytest.approx(0.3, abs=1e-15)
    a = np.pi / 4
    Rx, Ry = G.rotation([[np.cos(a / 2), np.sin(a / 2), 0, 0]]), G.rotation([[np.cos(a / 2), 0, np.sin(a / 2), 0]])
    zb = 0.8 * np.sqrt(2) - 0.02
    va, vb = G.vertices(0 * one, Rx, 0.4 * one), G.vertices([[0.05, 0.03, zb]], Ry, 0.4 * one)
    assert float(G.min_overlap(Rx, Ry, va, vb)[0]) == pytest.approx(0.02, abs=1e-15)
    assert float(G.surface_dist([[0.4, 0.1, -0.2]], 0 * one, R, 0.4 * one)[0]) == 0
    assert float(G.surface_dist([[0.1, 0.1, -0.2]], 0 * one, R, 0.4 * one)[0]) == pytest.approx(-0.2)
    hit, d, p, n = G.sphere_box_ref([[0, 0, 0.45]], [0.1], 0 * one, R, 0.4 * one)
    assert hit[0] and float(d[0]) == pytest.approx(-0.05) and np.allclose(p.astype(float), [[0, 0, 0.375]])
    assert np.array_equal(n.astype(float), [[0, 0, -1]])
    hit, d, p, n = G.sphere_box_ref([[0.1, 0, 0.3]], [0.1], 0 * one, R, 0.4 * one)
    assert hit[0] and float(d[0]) == pytest.approx(-0.2) and np.allclose(p.astype(float), [[0.1, 0, 0.3]])
    assert np.array_equal(n.astype(float), [[0, 0, -1]])


def test_oracle_world_records_are_the_narrowphase(oracle):
    """The pair lattice of tests/test_gpu_box_geometry.py through the oracle's
    own world: one step's records of both bodies of every pair equal
    kat_narrow of the same operands."""
    rows = G.lattice_rows(600)
    sc = G.pair_scene(rows)
    _, _, records = oracle.step(oracle.OracleScene(sc, max_partners=32), sc.qpos0, sc.qvel0, 1, record=True)
    assert set(records[2].tolist()) == set(G.KINDS)
    G.assert_records_are_the_narrowphase(records, oracle.kat_narrow(rows))
