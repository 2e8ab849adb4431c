"""The CPU model of the impulse query (rb_batch_impulses): one step of one
scene, contact by contact, made only of the oracle's pieces.

oracle.contacts gives the canonical per-body contact list of the state,
oracle.kat_inertia the world inertia, oracle.kat_impulse the two return values
of compute_collision_impulse_friction (collision.py:7-48) and the velocity
apply_impulse_friction (physics_utils.py:25-49) leaves.  The model is the
per-body Gauss-Seidel loop of the step (collision.py:72-88) around them:
gravity as v + (m g / m) dt in the real type, then for each contact of the body
in list order the step's skip rules (dist not below 0; |dist| < threshold) and
its normal (the frame flipped for the geom1 body under the oriented
convention), then kat_impulse on (m, e, mu, v, w, r = pos - x, n, I_w): its jn
and jt are the record, its v' and w' the next velocity.  net accumulates
P = jn n + jt and np_cross(r, P) element by element from +0 over the applied
contacts (un < 0).  For f32 the same in np.float32 with the oracle's f32
entries.

tests/test_impulse_model.py holds the model's velocity equal to oracle.step's
in every word; tests/test_gpu_batch_impulses.py holds the library to the model.
"""
from types import SimpleNamespace

import numpy as np

from oracle import oracle as O


def _self_is_geom1(kind_i, kind_j, i, j):
    """geom1 of a body pair: the sphere of a sphere-box pair, else the lower id
    (a plane is always geom1 of its contacts)."""
    if (kind_i == 0) != (kind_j == 0):
        return kind_i == 0
    return i < j


def impulses(sc, qpos, qvel, dt=None, restitution=None, friction=None, threshold=None, dtype="f64",
             max_partners=16):
    """One step's impulses for scene sc at state (qpos (M, 7), qvel (M, 6)).

    Returns a namespace: counts (M,) int32; partner, kind int32 and dist, jn
    (total,), jt (total, 3), flat over the bodies in order; vel, net (M, 6);
    applied, separating, skipped (by the threshold), apart (dist not below 0):
    how many records took each branch.  Reals are
    float64 arrays holding values of the real type."""
    T = np.float64 if dtype == "f64" else np.float32
    dt = T(sc.dt if dt is None else dt)
    e = sc.restitution if restitution is None else restitution
    mu = sc.friction if friction is None else friction
    thr = T(sc.threshold if threshold is None else threshold)
    osc = O.OracleScene(sc, max_partners=max_partners)
    M = sc.n
    q = np.ascontiguousarray(qpos, np.float64).reshape(M, 7)
    qv = np.ascontiguousarray(qvel, np.float64).reshape(M, 6)
    cnt, par, kin, dis, pos, frm = O.contacts(osc, q, dtype=dtype)
    Iw = O.kat_inertia(np.concatenate([np.asarray(sc.inertia, np.float64), q[:, 3:7]], axis=1), dtype=dtype)[:, :9]
    oriented = sc.normal_convention != "raw"
    g = np.asarray(sc.gravity, np.float64).astype(T)

    total = int(cnt.sum())
    jn_out, jt_out = np.zeros(total), np.zeros((total, 3))
    vel, net = np.zeros((M, 6)), np.zeros((M, 6))
    applied = separating = skipped = apart = 0
    c = 0
    for i in range(M):
        m = T(sc.mass[i])
        x = q[i, :3].astype(T)
        v = qv[i, :3].astype(T)
        w = qv[i, 3:].astype(T)
        F = m * g
        v = v + (F / m) * dt
        net_p, net_l = np.zeros(3, T), np.zeros(3, T)
        for _ in range(int(cnt[i])):
            d = T(dis[c])
            if not (d < 0):                      # collision.py:74
                apart += 1
                c += 1
                continue
            if abs(d) < thr:                     # collision.py:79-80
                skipped += 1
                c += 1
                continue
            j = int(par[c])
            flip = oriented and j >= 0 and _self_is_geom1(int(sc.kind[i]), int(sc.kind[j]), i, j)
            n = frm[c].astype(T)
            n = -n if flip else n
            r = pos[c].astype(T) - x
            row = np.concatenate([[m, e, mu], v, w, r, n, Iw[i]]).astype(np.float64)[None, :]
            out = O.kat_impulse(row, dtype=dtype)[0]
            jn, jt = T(out[0]), out[1:4].astype(T)
            jn_out[c], jt_out[c] = jn, jt
            v, w = out[4:7].astype(T), out[7:10].astype(T)
            # the function returns zeros exactly when the contact separates (un >= 0):
            # an approaching one has jn = -(1 + e) un / k > 0 (e >= 0)
            if jn == 0 and not jt.any():
                separating += 1
            else:
                applied += 1
                P = np.array([jn * n[0] + jt[0], jn * n[1] + jt[1], jn * n[2] + jt[2]], T)
                L = np.array([r[1] * P[2] - r[2] * P[1], r[2] * P[0] - r[0] * P[2], r[0] * P[1] - r[1] * P[0]], T)
                net_p = net_p + P
                net_l = net_l + L
            c += 1
        vel[i, :3], vel[i, 3:] = v, w
        net[i, :3], net[i, 3:] = net_p, net_l
    assert c == total
    return SimpleNamespace(counts=cnt.copy(), partner=par.copy(), kind=kin.copy(), dist=dis.copy(), jn=jn_out, jt=jt_out,
                           vel=vel, net=net, applied=applied, separating=separating, skipped=skipped, apart=apart)


def dense(m, R):
    """The model's records in the dense layout of the query, R slots per body:
    (counts (M,), partner, kind (M, R), dist, jn (M, R), jt (M, R, 3)); unused
    slots hold kind -1 and zeros, records past R are dropped."""
    M = m.counts.shape[0]
    partner, kind = np.zeros((M, R), np.int32), np.full((M, R), -1, np.int32)
    dist, jn, jt = np.zeros((M, R)), np.zeros((M, R)), np.zeros((M, R, 3))
    c = 0
    for i in range(M):
        k = min(int(m.counts[i]), R)
        partner[i, :k], kind[i, :k] = m.partner[c:c + k], m.kind[c:c + k]
        dist[i, :k], jn[i, :k], jt[i, :k] = m.dist[c:c + k], m.jn[c:c + k], m.jt[c:c + k]
        c += int(m.counts[i])
    return m.counts.copy(), partner, kind, dist, jn, jt


def words(a, dtype="f64"):
    """The words of reals of the real type held in a float64 array."""
    a = np.ascontiguousarray(a, np.float64)
    return a.view(np.uint64) if dtype == "f64" else np.ascontiguousarray(a.astype(np.float32)).view(np.uint32)
