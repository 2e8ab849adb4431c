"""The oracle against the heterogeneous goldens (tests/golden/make_golden.py,
the reference's own a1/a2/a3 functions): per-body radius, mass and
anisotropic inertia, three planes, gravity with x and y components and a
non-zero contact threshold (traj_mixed48, ORIENTED and RAW), and non-cubic
boxes lying on two planes at once (traj_bricks6).  Bit-exact, like
test_oracle_golden.py; plus the checks that these goldens really contain
what they are there for."""
import numpy as np
import pytest

from conftest import golden_scene, load_golden

MIXED_GOLDENS = ["traj_mixed48", "traj_mixed48_raw", "traj_bricks6"]


@pytest.mark.parametrize("name", MIXED_GOLDENS)
def test_mixed_trajectory_and_contacts_bit_exact(oracle, name):
    g = load_golden(name)
    sc = golden_scene(g)
    osc = oracle.OracleScene(sc)
    q, v = g["qpos0"], g["qvel0"]
    snaps = list(g["snap_step"])
    assert len(g["c_counts"]) == snaps[-1]          # contacts of every step
    si = 1
    for t in range(snaps[-1]):
        q, v, (cnt, par, kin, dis) = oracle.step(osc, q, v, 1, record=True)
        if t < len(g["c_counts"]):
            a, b = g["c_off"][t], g["c_off"][t + 1]
            assert np.array_equal(cnt, g["c_counts"][t]), f"contact counts differ at step {t}"
            assert np.array_equal(par, g["c_partner"][a:b]), f"contact partners differ at step {t}"
            assert np.array_equal(kin, g["c_kind"][a:b]), f"contact kinds differ at step {t}"
            assert np.array_equal(dis, g["c_dist"][a:b]), f"contact dists differ at step {t}"
        if si < len(snaps) and t + 1 == snaps[si]:
            assert np.array_equal(q, g["qpos"][si]), f"qpos differs at step {t + 1}"
            assert np.array_equal(v, g["qvel"][si]), f"qvel differs at step {t + 1}"
            si += 1
    assert si == len(snaps)


def _planes_per_body_step(g):
    """Number of distinct planes in each (step, body) contact list."""
    cnt = g["c_counts"].reshape(-1).astype(np.int64)
    par = g["c_partner"]
    owner = np.repeat(np.arange(cnt.size), cnt)
    pl = par < 0
    pairs = np.unique(np.stack([owner[pl], par[pl].astype(np.int64)], axis=1), axis=0)
    return np.bincount(pairs[:, 0], minlength=cnt.size)


@pytest.mark.parametrize("name", ["traj_mixed48", "traj_mixed48_raw"])
def test_mixed_goldens_are_heterogeneous_and_multi_plane(name):
    g = load_golden(name)
    kin, par, dis = g["c_kind"], g["c_partner"], g["c_dist"]
    assert set(np.unique(kin).tolist()) == {0, 16}
    assert (_planes_per_body_step(g) >= 2).sum() >= 50
    assert np.unique(par[par < 0]).size >= 3 and g["planes"].shape[0] == 3
    # a sphere-sphere contact shallower than the threshold was skipped
    thr = float(g["params"][3])
    assert thr == 1e-4 and ((kin == 16) & (dis < 0) & (dis > -thr)).any()
    # and so was a plane contact
    assert ((kin == 0) & (dis < 0) & (dis > -thr)).any()
    # every body its own radius, mass and three different principal inertias
    n = g["mass"].size
    assert np.unique(g["mass"]).size == n and np.unique(g["size"][:, 0]).size == n
    I = g["inertia"]
    assert ((I[:, 0] != I[:, 1]) & (I[:, 1] != I[:, 2]) & (I[:, 0] != I[:, 2])).all()
    assert g["size"][:, 0].max() / g["size"][:, 0].min() <= 2.0
    assert g["gravity"][0] != 0 and g["gravity"][1] != 0
    # the orientations are not the identity, so R I R^T differs from I
    assert (np.abs(g["qpos0"][:, 4:7]).max(axis=1) > 0.1).all()


def test_bricks_golden_has_every_corner_and_both_planes():
    g = load_golden("traj_bricks6")
    kin, par = g["c_kind"], g["c_partner"]
    assert set(np.unique(kin).tolist()) == set(range(1, 9))
    assert set(np.unique(par).tolist()) == {-1, -2}
    assert (_planes_per_body_step(g) == 2).sum() >= 100
    s, I = g["size"], g["inertia"]
    assert ((s[:, 0] != s[:, 1]) & (s[:, 1] != s[:, 2]) & (s[:, 0] != s[:, 2])).all()
    assert ((I[:, 0] != I[:, 1]) & (I[:, 1] != I[:, 2]) & (I[:, 0] != I[:, 2])).all()
    assert np.unique(g["mass"]).size == g["mass"].size
    assert g["gravity"][1] != 0
    # plane order, then corners in bit order, at most 4 per plane: within a
    # body's list the plane index never goes back, and per plane the corner
    # kinds ascend
    cnt = g["c_counts"].reshape(-1)
    off = np.concatenate([[0], np.cumsum(cnt)])
    full = 0
    for i in np.flatnonzero(cnt >= 2):
        p, k = -1 - par[off[i]:off[i + 1]], kin[off[i]:off[i + 1]]
        key = p * 16 + k
        assert (np.diff(key) > 0).all(), (p, k)
        assert np.bincount(p).max() <= 4
        full += int(np.bincount(p).max() == 4)
    assert full > 0                                   # a face lay flat: the 4-corner cap was reached


def test_generators_reproduce_the_goldens_scenes():
    """scenes.mixed_spheres / trough_bricks still draw the committed goldens'
    scenes, so the GPU tests' larger scenes are of the same family."""
    from rbhip import scenes
    for name, sc in (("traj_mixed48", scenes.mixed_spheres(8, 6, seed=1)),
                     ("traj_bricks6", scenes.trough_bricks(6, seed=2))):
        g = load_golden(name)
        for key, val in (("kind", sc.kind), ("mass", sc.mass), ("inertia", sc.inertia), ("size", sc.size),
                         ("planes", sc.planes), ("gravity", sc.gravity), ("qpos0", sc.qpos0), ("qvel0", sc.qvel0)):
            assert np.array_equal(g[key], val), (name, key)
        assert np.array_equal(g["params"], [sc.dt, sc.restitution, sc.friction, sc.threshold])


def test_mixed_types_argument():
    """types=k draws each body's (m, I) from k rows; types=None gives every
    body its own."""
    from rbhip import scenes
    for k in (3, 4, 5):
        sc = scenes.mixed_spheres(64, 64, seed=3, types=k)
        rows = np.unique(np.concatenate([sc.mass[:, None], sc.inertia], axis=1), axis=0)
        assert rows.shape[0] == k
    sc = scenes.mixed_spheres(37, 29, seed=3)
    assert sc.n == 1073 and np.unique(sc.mass).size == sc.n
