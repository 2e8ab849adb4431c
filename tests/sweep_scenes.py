"""Shared by the per-environment batch tests (test_oracle_sweep_golden.py,
test_gpu_batch_env.py): the scenes of the two sweep goldens, one per
environment, and the oracle run on a list of scenes with applied forces."""
import numpy as np

from conftest import golden_scene


def sweep_scenes(g):
    """One Scene per environment of a sweep golden (make_golden_sweep.py): the
    shared arrays with the environment's own planes, gravity, restitution,
    friction and start state where the file has them."""
    base = golden_scene(g)
    E = g["env_qpos0"].shape[0]
    scs = []
    for k in range(E):
        kw = dict(planes=g["env_planes"][k], qpos0=g["env_qpos0"][k], qvel0=g["env_qvel0"][k])
        if "env_gravity" in g:
            kw["gravity"] = g["env_gravity"][k]
        if "env_restitution" in g:
            kw["restitution"] = float(g["env_restitution"][k])
            kw["friction"] = float(g["env_friction"][k])
        scs.append(base.with_(**kw))
    return scs


def oracle_envs(oracle, scs, q, v, steps, dtype="f64", keep=(), xfrc=None, max_partners=16):
    """Each environment k through the oracle on its own scene scs[k] (with
    xfrc[k] as its applied forces when xfrc is given), one step at a time so
    that every step's recorded contact list is seen.  Returns the final
    (E, M, 7) / (E, M, 6) state, the states after the step counts in `keep`
    and the counts of what was recorded: per environment the plane records
    ("plane": kinds 0..8) and sphere-sphere records ("ss": kind 16), and over
    all environments the body-steps with records on two or more planes
    ("multi")."""
    q, v = np.array(q, np.float64), np.array(v, np.float64)
    E = len(scs)
    kept = {t: (q.copy(), v.copy()) for t in keep}
    stats = dict(plane=np.zeros(E, np.int64), ss=np.zeros(E, np.int64), multi=0)
    for k, sc in enumerate(scs):
        osc = oracle.OracleScene(sc, max_partners=max_partners)
        xf = None if xfrc is None else xfrc[k]
        qq, vv = q[k], v[k]
        for t in range(1, steps + 1):
            qq, vv, (cnt, par, kin, dis) = oracle.step(osc, qq, vv, 1, dtype=dtype, xfrc=xf, record=True)
            stats["ss"][k] += int((kin == 16).sum())
            stats["plane"][k] += int((kin < 16).sum())
            off = np.concatenate([[0], np.cumsum(cnt)])
            for i in range(sc.n):
                p = par[off[i]:off[i + 1]]
                if len(np.unique(p[p < 0])) >= 2:
                    stats["multi"] += 1
            if t in kept:
                kept[t][0][k], kept[t][1][k] = qq, vv
        q[k], v[k] = qq, vv
    return q, v, kept, stats
