// rb_balls.hpp — the two-ball law (src/simulation/ball_collision.py), each
// part written once: impulse, ground phase, reach test, and the evaluation of
// a pair (ball_pair).  The world's kernels (rb_balls.hip) and the batch kernel
// (rb_batch.hip) differ only in where a ball's partners come from, so a batch
// and a world agree bit for bit (as rb_device.hpp / rb_body.hpp for the default law).
#pragma once
#include "rb_device.hpp"
#include "rb_internal.hpp"

namespace rb {

// ball_collision.py:53-68
template <typename T>
__device__ __forceinline__ V3<T> pair_impulse(T mass, const M3<T> &Iinv, V3<T> v, V3<T> w, V3<T> r, V3<T> n, T e,
                                              T mu) {
    const V3<T> c = np_cross(w, r);
    const V3<T> vc = {v.x + c.x, v.y + c.y, v.z + c.z};                     // :54
    const T vn = np_dot(vc, n);                                             // :55
    const V3<T> vt = {vc.x - vn * n.x, vc.y - vn * n.y, vc.z - vn * n.z};   // :56
    const T tn = sqroot(np_dot(vt, vt));                                    // :57
    const V3<T> axr = np_cross(np_matvec(Iinv, np_cross(r, n)), r);
    const T dn = (T(1) / mass) + np_dot(n, axr);                            // :59
    const T jn = (-(T(1) + e) * vn) / dn;                                   // :60
    V3<T> td = {T(0), T(0), T(0)};
    if (tn > T(1e-8)) td = {vt.x / tn, vt.y / tn, vt.z / tn};               // :62
    const V3<T> bxr = np_cross(np_matvec(Iinv, np_cross(r, td)), r);
    const T dtn = (T(1) / mass) + np_dot(td, bxr);                          // :63-64
    const T jtu = -tn / dtn;                                                // :65
    const T lim = mu * absval(jn);
    T jt = jtu > -lim ? jtu : -lim;                                         // :66 np.clip
    jt = jt < lim ? jt : lim;
    return {jn * n.x + jt * td.x, jn * n.y + jt * td.y, jn * n.z + jt * td.z};   // :68
}

// ball_collision.py:39-41
template <typename T> __device__ __forceinline__ M3<T> ball_iinv(T m, T r) {
    const T I = (T(0.4) * m) * (r * r);
    M3<T> A;
#pragma unroll
    for (int k = 0; k < 9; ++k) A.a[k] = (k % 4 == 0) ? T(1) / I : T(0) / I;
    return A;
}

// gravity and the ground contact of one ball (ball_collision.py:77-97)
template <typename T>
__device__ __forceinline__ void ball_ground(const StepParams<T> &p, V3<T> &x, V3<T> &v, V3<T> &w, T m, T rad,
                                            const M3<T> &Iinv) {
    v = {v.x + p.g[0] * p.dt, v.y + p.g[1] * p.dt, v.z + p.g[2] * p.dt};   // :78
    if (!p.ground || !(x.z < rad)) return;                                  // :90
    const V3<T> n = {T(0), T(0), T(1)};                                     // :88
    const V3<T> cp = {x.x - rad * n.x, x.y - rad * n.y, x.z - rad * n.z};   // :91
    const V3<T> rr = {cp.x - x.x, cp.y - x.y, cp.z - x.z};                  // :92
    const V3<T> imp = pair_impulse(m, Iinv, v, w, rr, n, p.e, p.mu);        // :93-94
    const V3<T> dw = np_matvec(Iinv, np_cross(rr, imp));
    v = {v.x + imp.x / m, v.y + imp.y / m, v.z + imp.z / m};                // :95
    w = {w.x + dw.x, w.y + dw.y, w.z + dw.z};                               // :96
    x.z = rad;                                                              // :97
}

// |p_b - p_a| < r_a + r_b + tol for the pair (a < b), ball_collision.py:100-103
// (decided on the squared distance when clear of the threshold, see
// sphere_sphere_hit)
template <typename T> __device__ __forceinline__ bool ball_hit(V3<T> pa, T ra, V3<T> pb, T rb, T tol) {
    const V3<T> d = {pb.x - pa.x, pb.y - pa.y, pb.z - pa.z};
    const T d2 = np_dot(d, d);
    const T L = (ra + rb) + tol;
    const T L2 = L * L;
    if (RB_SQ_PREFILTER) {
        if (d2 > L2 * (T(1) + sq_margin<T>())) return false;
        if (d2 < L2 * (T(1) - sq_margin<T>())) return true;
    }
    return sqroot(d2) < L;
}

// One pair within reach, from the post-ground state of both balls, as the
// calling ball sees it (ball_collision.py:100-118).  The ball of the lower id
// is a (self_a: the caller is); the impulse is the one from a's side, applied
// + to a and - to b, and the positions are pushed apart by half the overlap.
// Adds the caller's share to its running x, v, w; returns |p_b - p_a|.
template <typename T>
__device__ __forceinline__ T ball_pair(V3<T> xo, V3<T> vo, V3<T> wo, T mi, T ri, const M3<T> &Ii, V3<T> xj, V3<T> vj,
                                       V3<T> wj, T mj, T rj, bool self_a, T e, T mu, T tol, V3<T> &x, V3<T> &v,
                                       V3<T> &w) {
    const V3<T> pa = self_a ? xo : xj, pb = self_a ? xj : xo;
    const V3<T> va = self_a ? vo : vj, wa = self_a ? wo : wj;
    const T ma = self_a ? mi : mj, ra = self_a ? ri : rj, rb = self_a ? rj : ri;
    const M3<T> Ia = self_a ? Ii : ball_iinv(mj, rj);
    const V3<T> diff = {pb.x - pa.x, pb.y - pa.y, pb.z - pa.z};             // :100
    const T dist = sqroot(np_dot(diff, diff));                              // :101
    const T dd = dist + T(1e-8);
    const V3<T> n = {diff.x / dd, diff.y / dd, diff.z / dd};                // :104
    const V3<T> cp = {(pa.x + pb.x) / T(2), (pa.y + pb.y) / T(2), (pa.z + pb.z) / T(2)};   // :105
    const V3<T> r1 = {cp.x - pa.x, cp.y - pa.y, cp.z - pa.z};               // :106
    const V3<T> imp = pair_impulse(ma, Ia, va, wa, r1, n, e, mu);           // :109-110
    const T corr = (((ra + rb) + tol) - dist) / T(2);                       // :116
    if (self_a) {
        const V3<T> dw = np_matvec(Ii, np_cross(r1, imp));
        v = {v.x + imp.x / mi, v.y + imp.y / mi, v.z + imp.z / mi};         // :111
        w = {w.x + dw.x, w.y + dw.y, w.z + dw.z};                           // :112
        x = {x.x - corr * n.x, x.y - corr * n.y, x.z - corr * n.z};         // :117
    } else {
        const V3<T> r2 = {cp.x - pb.x, cp.y - pb.y, cp.z - pb.z};           // :107
        const V3<T> dw = np_matvec(Ii, np_cross(r2, imp));
        v = {v.x - imp.x / mi, v.y - imp.y / mi, v.z - imp.z / mi};         // :113
        w = {w.x - dw.x, w.y - dw.y, w.z - dw.z};                           // :114
        x = {x.x + corr * n.x, x.y + corr * n.y, x.z + corr * n.z};         // :118
    }
    return dist;
}

}  // namespace rb
