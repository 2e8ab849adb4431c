// rb_body.hpp — the per-body law, once: the pieces of the step shared by the
// hashed-cell step kernels (rb_step.hpp: body_update and the helper wave's
// help_body), the cell-ordered tile kernel (rb_tiles.hip) and the batched
// worlds (rb_batch.hip): contact recording, the lazily evaluated world
// inverse inertia, one contact through the reference's skip rules and
// impulse (K2), gravity / applied forces (a4), a body's plane contacts and
// its sphere-sphere pair (K2), and the integration of position and
// orientation (K3).  The operation order is the reference's
// (rb_device.hpp), so every kernel that calls these steps a body
// bit-identically.
#pragma once

#include "rb_device.hpp"
#include "rb_internal.hpp"

#ifndef RB_ABLATE
#define RB_ABLATE 0
#endif

namespace rb {

template <typename T>
__device__ __forceinline__ void record(const StepParams<T> &p, int32_t l, int32_t &nrec, int32_t partner,
                                       int32_t kind, T dist) {
    if (!p.rec_count) return;
    if (nrec < p.maxrec) {
        const int64_t o = (int64_t)l * p.maxrec + nrec;
        p.rec_partner[o] = partner;
        p.rec_kind[o] = kind;
        p.rec_dist[o] = dist;
    }
    ++nrec;
}

// Lazily evaluated inv(inertia_world): the reference computes it every step
// (collision.py:62) but it only reaches the state through a torque or an
// applied impulse; computing it on first use is value-identical and keeps
// it out of the broadphase's register live range.
template <typename T> struct LazyInvI {
    V3<T> I;
    Q4<T> q;
    bool have = false;
    M3<T> m;
    __device__ __forceinline__ const M3<T> &get() {
        if (!have) {
#if RB_ABLATE == 2
            for (int k = 0; k < 9; ++k) m.a[k] = (k % 4 == 0) ? T(1) / I.x : T(0);
#else
            m = np_inv3(inertia_world(I, q));
#endif
            have = true;
        }
        return m;
    }
};

// one contact of body i through the reference's skip rules then K2
template <typename T>
__device__ __forceinline__ void solve_contact(const StepParams<T> &p, const Contact<T> &con, V3<T> x, V3<T> n,
                                              T m, T k, LazyInvI<T> &invI, V3<T> &v, V3<T> &w) {
    if (!(con.dist < T(0))) return;                 // collision.py:74 (NaN fails too)
    if (absval(con.dist) < p.thr) return;           // collision.py:79-80
    const V3<T> r = {con.pos.x - x.x, con.pos.y - x.y, con.pos.z - x.z};   // :75
    T jn;
    V3<T> jt;
    if (impulse(k, v, w, r, n, p.e, p.mu, jn, jt)) apply(v, w, m, invI.get(), r, n, jn, jt);
}

// a4 (collision.py:66-70): gravity plus the optional applied force / torque
// (XFRC false: a caller whose worlds never carry one, so no branch on it)
template <typename T, bool XFRC = true>
__device__ __forceinline__ void apply_force(const StepParams<T> &p, int32_t l, T m, LazyInvI<T> &invI, V3<T> &v,
                                            V3<T> &w) {
    V3<T> F = {m * p.g[0], m * p.g[1], m * p.g[2]};
    if (XFRC && p.xfrc) F = {p.xfrc[l] + F.x, p.xfrc[p.S + l] + F.y, p.xfrc[2 * p.S + l] + F.z};
    v = {v.x + (F.x / m) * p.dt, v.y + (F.y / m) * p.dt, v.z + (F.z / m) * p.dt};
    if (XFRC && p.xfrc) {
        const V3<T> tdt = {p.xfrc[3 * p.S + l] * p.dt, p.xfrc[4 * p.S + l] * p.dt, p.xfrc[5 * p.S + l] * p.dt};
        const V3<T> dw = np_matvec(invI.get(), tdt);
        w = {w.x + dw.x, w.y + dw.y, w.z + dw.z};
    }
}
// a4 with the body's applied force xf and torque xt given by value (a caller
// that holds them in registers: the batched worlds): the XFRC path above, in
// its order, all-zero rows included
template <typename T>
__device__ __forceinline__ void apply_force(const StepParams<T> &p, T m, LazyInvI<T> &invI, V3<T> &v, V3<T> &w,
                                            V3<T> xf, V3<T> xt) {
    V3<T> F = {m * p.g[0], m * p.g[1], m * p.g[2]};
    F = {xf.x + F.x, xf.y + F.y, xf.z + F.z};
    v = {v.x + (F.x / m) * p.dt, v.y + (F.y / m) * p.dt, v.z + (F.z / m) * p.dt};
    const V3<T> tdt = {xt.x * p.dt, xt.y * p.dt, xt.z * p.dt};
    const V3<T> dw = np_matvec(invI.get(), tdt);
    w = {w.x + dw.x, w.y + dw.y, w.z + dw.z};
}

// K2, a body's plane contacts, the first in its contact order: plane order,
// a sphere's one per plane, a box's corners (8, at most 4 per plane).
// pl carries the planes (n_planes, pn, pp): the step's parameters, or the
// batch's next to its per-environment StepParams.  l: the body's row of the
// contact records.
template <typename T, typename Planes>
__device__ __forceinline__ void solve_planes_sphere(const StepParams<T> &p, const Planes &pl, int32_t l, V3<T> x,
                                                    T rad, T m, T k, LazyInvI<T> &invI, V3<T> &v, V3<T> &w,
                                                    int32_t &nrec) {
    for (int a = 0; a < pl.n_planes; ++a) {
        const V3<T> pn = {pl.pn[a][0], pl.pn[a][1], pl.pn[a][2]};
        const V3<T> pp = {pl.pp[a][0], pl.pp[a][1], pl.pp[a][2]};
        Contact<T> con;
        if (!plane_sphere(pn, pp, x, rad, con)) continue;
        record(p, l, nrec, -1 - a, 0, con.dist);
        solve_contact(p, con, x, con.frame, m, k, invI, v, w);
    }
}
// M: the box's orientation (mj_body_mat of its quaternion), sz: its half extents
template <typename T, typename Planes>
__device__ __forceinline__ void solve_planes_box(const StepParams<T> &p, const Planes &pl, int32_t l, V3<T> x,
                                                 const M3<T> &M, V3<T> sz, T m, T k, LazyInvI<T> &invI, V3<T> &v,
                                                 V3<T> &w, int32_t &nrec) {
    for (int a = 0; a < pl.n_planes; ++a) {
        const V3<T> pn = {pl.pn[a][0], pl.pn[a][1], pl.pn[a][2]};
        const V3<T> dif = {x.x - pl.pp[a][0], x.y - pl.pp[a][1], x.z - pl.pp[a][2]};
        const T dist = mj_dot(dif, pn);
        int cnt = 0;
        for (int c = 0; c < 8 && cnt < 4; ++c) {
            Contact<T> con;
            if (!plane_box_corner(pn, x, dist, M, sz, c, con)) continue;
            ++cnt;
            record(p, l, nrec, -1 - a, 1 + c, con.dist);
            solve_contact(p, con, x, con.frame, m, k, invI, v, w);
        }
    }
}

// K2, the sphere-sphere pair of body i (centre x, radius r) with partner j
// (step-start centre cj, radius rj): MuJoCo's geom order is by id, and the
// contact frame points from geom1 to geom2
template <typename T>
__device__ __forceinline__ void solve_sphere_pair(const StepParams<T> &p, int32_t l, int32_t i, int32_t j, V3<T> x,
                                                  T r, V3<T> cj, T rj, T m, T k, LazyInvI<T> &invI, V3<T> &v,
                                                  V3<T> &w, int32_t &nrec) {
    Contact<T> con;
    V3<T> n;
    if (i < j) {                        // this body is geom1
        sphere_sphere(x, r, cj, rj, con);
        n = p.oriented ? V3<T>{-con.frame.x, -con.frame.y, -con.frame.z} : con.frame;
    } else {
        sphere_sphere(cj, rj, x, r, con);
        n = con.frame;
    }
    record(p, l, nrec, j, 16, con.dist);
    solve_contact(p, con, x, n, m, k, invI, v, w);
}

// K3 (collision.py:90-100): x += v dt; q += 0.5 (0, w) q dt, normalised.
// Two halves: the hashed step kernels claim the next table's slot between
// them (rb_step.hpp body_update)
template <typename T> __device__ __forceinline__ void integrate_position(V3<T> &x, V3<T> v, T dt) {
    x = {x.x + v.x * dt, x.y + v.y * dt, x.z + v.z * dt};
}
template <typename T>
__device__ __forceinline__ void integrate_orientation(Q4<T> &qn, const Q4<T> &q, V3<T> w, T dt) {
    const Q4<T> res = mj_mulquat(Q4<T>{T(0), w.x, w.y, w.z}, q);
    qn = {q.w + (T(0.5) * res.w) * dt, q.x + (T(0.5) * res.x) * dt, q.y + (T(0.5) * res.y) * dt,
          q.z + (T(0.5) * res.z) * dt};
    const T nq = sqroot(fmadd(qn.z, qn.z, fmadd(qn.y, qn.y, fmadd(qn.x, qn.x, qn.w * qn.w))));
    qn = {qn.w / nq, qn.x / nq, qn.y / nq, qn.z / nq};
}
template <typename T>
__device__ __forceinline__ void integrate_pose(V3<T> &x, Q4<T> &qn, const Q4<T> &q, V3<T> v, V3<T> w, T dt) {
    integrate_position(x, v, dt);
    integrate_orientation(qn, q, w, dt);
}

}  // namespace rb
