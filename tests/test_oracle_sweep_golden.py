"""The per-environment sweep goldens (tests/golden/make_golden_sweep.py: the
reference's own functions on a cube-incline angle sweep and on four balls
with per-environment planes, gravity and applied forces) against the oracle,
value for value; and the scene constructors and BatchWorld.from_scenes checks
that need no GPU."""
import numpy as np
import pytest

from conftest import load_golden
from sweep_scenes import sweep_scenes


def test_cube_incline_sweep_bit_exact(oracle):
    """timestep_integration on cube_incline(a), a = 0.0 .. 0.7, every stored step."""
    g = load_golden("sweep_cube_incline")
    scs = sweep_scenes(g)
    snaps = list(g["snap_step"])
    assert len(scs) == 8 and snaps[-1] == 300
    for k, sc in enumerate(scs):
        osc = oracle.OracleScene(sc)
        q, v = sc.qpos0, sc.qvel0
        for si in range(1, len(snaps)):
            q, v = oracle.step(osc, q, v, int(snaps[si] - snaps[si - 1]))
            assert np.array_equal(q, g["qpos"][k, si]), f"angle {g['angles'][k]}: qpos differs at step {snaps[si]}"
            assert np.array_equal(v, g["qvel"][k, si]), f"angle {g['angles'][k]}: qvel differs at step {snaps[si]}"
    # the sweep is one: the final states differ pairwise
    fin = g["qpos"][:, -1, 0, :]
    assert len({fin[k].tobytes() for k in range(8)}) == 8


def test_cube_incline_sweep_ends_in_the_single_cube_golden():
    """The 0.7 rad environment is models/cube.xml's own scene: the first 300
    steps of traj_single_cube."""
    g = load_golden("sweep_cube_incline")
    c = load_golden("traj_single_cube")
    assert g["angles"][7] == 0.7
    for si, t in enumerate(g["snap_step"]):
        assert np.array_equal(g["qpos"][7, si, 0], c["qpos"][t]) and np.array_equal(g["qvel"][7, si, 0], c["qvel"][t])


def test_balls4_env_bit_exact(oracle):
    """nbody_step on 8 environments of four balls, each with its own two
    planes, gravity, restitution, friction and constant xfrc_applied."""
    g = load_golden("sweep_balls4_env")
    scs = sweep_scenes(g)
    snaps = list(g["snap_step"])
    assert len(scs) == 8 and snaps[-1] == 200 and g["env_planes"].shape == (8, 2, 6)
    ss = plane = 0
    for k, sc in enumerate(scs):
        osc = oracle.OracleScene(sc)
        q, v = sc.qpos0, sc.qvel0
        si = 1
        for t in range(1, snaps[-1] + 1):
            q, v, (cnt, par, kin, dis) = oracle.step(osc, q, v, 1, xfrc=g["env_xfrc"][k], record=True)
            ss += int((kin == 16).sum())
            plane += int((kin == 0).sum())
            if t == snaps[si]:
                assert np.array_equal(q, g["qpos"][k, si]), f"environment {k}: qpos differs at step {t}"
                assert np.array_equal(v, g["qvel"][k, si]), f"environment {k}: qvel differs at step {t}"
                si += 1
    # the balls met each other and the planes, and the forces did something
    assert ss >= 8 and plane >= 80, (ss, plane)
    q0, _ = oracle.step(oracle.OracleScene(scs[0]), scs[0].qpos0, scs[0].qvel0, 10)
    assert not np.array_equal(q0, g["qpos"][0, 1])


def test_cube_incline_at_the_model_angle_is_single_cube():
    from rbhip import scenes
    a, b = scenes.cube_incline(0.7), scenes.single_cube()
    for f in ("kind", "mass", "inertia", "size", "planes", "qpos0", "qvel0", "gravity"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f
    assert (a.dt, a.restitution, a.friction, a.threshold, a.normal_convention) == \
           (b.dt, b.restitution, b.friction, b.threshold, b.normal_convention)
    # other angles: the plane normal (0, -sin a, cos a) and the start quaternion (cos a/2, sin a/2, 0, 0)
    c = scenes.cube_incline(0.25)
    assert np.array_equal(c.planes, [[0.0, -np.sin(0.25), np.cos(0.25), 0.0, 0.0, 0.0]])
    assert np.array_equal(c.qpos0, [[0.0, 0.0, 0.4, np.cos(0.125), np.sin(0.125), 0.0, 0.0]])
    s, s0 = scenes.sphere_incline(0.25), scenes.single_sphere()
    assert np.array_equal(s.planes, c.planes)
    assert np.array_equal(s.qpos0, s0.qpos0) and np.array_equal(s.qvel0, s0.qvel0) and s.kind[0] == scenes.SPHERE
    assert np.array_equal(scenes.sphere_incline(0.0).planes, s0.planes)


def test_from_scenes_refuses_mismatched_scenes(monkeypatch):
    """Scenes that disagree in body count, kinds, plane count, dt, threshold
    or normal convention: ValueError naming the first offender, before any
    batch is created (the constructor is a stub that must not be reached)."""
    from rbhip import BatchWorld, scenes

    def no_batch(self, *a, **kw):
        raise AssertionError("a batch was created")

    monkeypatch.setattr(BatchWorld, "__init__", no_batch)
    c = scenes.cube_incline
    two_planes = np.concatenate([c(0.2).planes, c(0.3).planes])
    for bad, what in ((scenes.multi_sphere4(), "body count"),
                      (scenes.sphere_incline(0.1), "kinds"),
                      (c(0.2).with_(planes=two_planes), "plane count"),
                      (c(0.2).with_(dt=0.01), "dt"),
                      (c(0.2).with_(threshold=0.0), "threshold"),
                      (c(0.2).with_(normal_convention="raw"), "normal convention")):
        with pytest.raises(ValueError, match=f"scene 2 .*{what}"):
            BatchWorld.from_scenes([c(0.0), c(0.1), bad, bad])
    with pytest.raises(ValueError):
        BatchWorld.from_scenes([])
    # matching scenes reach the constructor
    with pytest.raises(AssertionError, match="a batch was created"):
        BatchWorld.from_scenes([c(0.0), c(0.1)])
