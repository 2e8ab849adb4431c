"""Generate the per-environment sweep goldens (sweep_cube_incline.npz,
sweep_balls4_env.npz) from the REFERENCE's own Python functions, with the
helpers of make_golden.py (the stub `mujoco`, Model / Data, the N-body
driver).  Like make_golden.py it runs only where the read-only reference
checkout is; the .npz outputs are committed and are what tests read.  Usage:

    python tests/golden/make_golden_sweep.py --reference <reference checkout>

sweep_cube_incline: src/physics/time_integeration.py:13-72 timestep_integration
on scenes.cube_incline(a) for a = 0.0, 0.1, ..., 0.7 — the knob
INCLINE_ANGLE_RAD of src/config/sim_overrides.py, which
src/simulation/cube_incline.py:28-34 writes into the model (plane and start
orientation) — 300 steps, states every 10 steps.

sweep_balls4_env: 8 environments of multi_sphere4 stepped with nbody_step
(multi_sphere_bounce.py:42-92), 200 steps, states every 10 steps.  Every
environment has its own two planes (a V trough through the origin), gravity,
restitution, friction and a constant data.xfrc_applied per body (set on Data
before the loop; collision.py:66-70 reads it every step); the balls start
moved together so that they meet.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import Data, Model, install_stub, nbody_step, run_single, scene_arrays, scenes  # noqa: E402

ANGLES = np.arange(8) / 10.0          # (7 / 10 is the 0.7 of models/cube.xml; 7 * 0.1 is not)
CUBE_STEPS, BALL_STEPS, EVERY = 300, 200, 10
BALL_ENVS = 8


def balls4_env_inputs():
    """The per-environment arrays of sweep_balls4_env (seed 4242)."""
    sc = scenes.multi_sphere4()
    E = BALL_ENVS
    rng = np.random.default_rng(4242)
    q = np.zeros((E, 4, 7))
    q[:, :, 0:2] = np.sign(sc.qpos0[:, 0:2]) * 0.095 + rng.uniform(-0.01, 0.01, (E, 4, 2))
    q[:, :, 2] = 0.5 + 0.3 * rng.uniform(0.0, 1.0, (E, 4))
    q[:, :, 3] = 1.0
    v = np.zeros((E, 4, 6))
    v[:, :, 0:3] = rng.normal(0.0, 0.3, (E, 4, 3))
    v[:, :, 3:6] = rng.normal(0.0, 1.0, (E, 4, 3))
    e = rng.uniform(0.2, 1.0, E)
    mu = rng.uniform(0.0, 0.8, E)
    a, b = rng.uniform(0.05, 0.4, E), rng.uniform(0.05, 0.4, E)
    planes = np.zeros((E, 2, 6))
    planes[:, 0, 0], planes[:, 0, 2] = np.sin(a), np.cos(a)
    planes[:, 1, 0], planes[:, 1, 2] = -np.sin(b), np.cos(b)
    gravity = np.stack([rng.uniform(-0.5, 0.5, E), rng.uniform(-0.5, 0.5, E), -9.8 * rng.uniform(0.5, 1.5, E)], axis=1)
    xfrc = np.concatenate([rng.normal(0.0, 0.2, (E, 4, 3)), rng.normal(0.0, 0.01, (E, 4, 3))], axis=2)
    return sc, q, v, e, mu, planes, gravity, xfrc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    args = ap.parse_args()
    install_stub()
    sys.path.insert(0, args.reference)
    from src.physics import collision as ref_collision
    from src.physics import physics_utils as ref_utils
    from src.physics import time_integeration as ref_ti

    class Ref:
        compute_collision_impulse_friction = staticmethod(ref_collision.compute_collision_impulse_friction)
        apply_impulse_friction = staticmethod(ref_utils.apply_impulse_friction)
        compute_inertia_tensor_world = staticmethod(ref_collision.compute_inertia_tensor_world)

    snap = np.arange(0, CUBE_STEPS + 1, EVERY)
    scs = [scenes.cube_incline(float(a)) for a in ANGLES]
    qs, vs = [], []
    for sc in scs:
        q, v, _ = run_single(ref_ti.timestep_integration, sc, "cube", CUBE_STEPS,
                             restitution=sc.restitution, friction_coeff=sc.friction)
        qs.append(q[snap][:, None, :])
        vs.append(v[snap][:, None, :])
    np.savez_compressed(os.path.join(HERE, "sweep_cube_incline.npz"), angles=ANGLES, snap_step=snap,
                        qpos=np.array(qs), qvel=np.array(vs),
                        env_planes=np.array([sc.planes for sc in scs]),
                        env_qpos0=np.array([sc.qpos0 for sc in scs]),
                        env_qvel0=np.array([sc.qvel0 for sc in scs]), **scene_arrays(scs[0]))
    print("sweep_cube_incline done")

    sc, q0, v0, e, mu, planes, gravity, xfrc = balls4_env_inputs()
    snap = np.arange(0, BALL_STEPS + 1, EVERY)
    qs = np.zeros((BALL_ENVS, len(snap), 4, 7))
    vs = np.zeros((BALL_ENVS, len(snap), 4, 6))
    for k in range(BALL_ENVS):
        sk = sc.with_(planes=planes[k], gravity=gravity[k], restitution=float(e[k]), friction=float(mu[k]),
                      qpos0=q0[k], qvel0=v0[k])
        model = Model(sk)
        data = Data(model)
        data.xfrc_applied[model.first:] = xfrc[k]
        qs[k, 0], vs[k, 0] = q0[k], v0[k]
        for t in range(1, BALL_STEPS + 1):
            nbody_step(Ref(), model, data, sk.dt, sk.restitution, sk.friction, sk.threshold, sk.normal_convention)
            if t % EVERY == 0:
                qs[k, t // EVERY] = data.qpos.reshape(4, 7)
                vs[k, t // EVERY] = data.qvel.reshape(4, 6)
    assert np.isfinite(qs).all() and np.isfinite(vs).all()
    np.savez_compressed(os.path.join(HERE, "sweep_balls4_env.npz"), snap_step=snap, qpos=qs, qvel=vs,
                        env_planes=planes, env_gravity=gravity, env_xfrc=xfrc, env_restitution=e, env_friction=mu,
                        env_qpos0=q0, env_qvel0=v0, **scene_arrays(sc))
    print("sweep_balls4_env done")


if __name__ == "__main__":
    main()
