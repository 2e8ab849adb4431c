// rb_contacts.hpp — the records of the contact queries (the batch's,
// rb_batch_contacts.hip and rb_batch_wide.hip; a world's, rb_world_contacts.hip):
// one copy of the record writer for all three, and the walk over the planes
// and the emission of one pair as the world's query runs them.
//
// The batch kernels keep the walk and the pair emission in line
// (contacts_body, wide_contacts_kernel, ragged_contacts_body).  Moved onto one
// body built on contacts_planes / contacts_pair below they produce the same
// lists in fewer registers (the box instances 232 -> 181 at f64, 162 -> 134 at
// f32), and the mixed template's query of 1,024 environments took 32.6-33.4 us
// a call against 31.9-32.2 in an alternating run, so they stay as they are
// (cause not found; DESIGN 4.3, profiles/batch_unify).  The order, the geom1
// rule and the tests are the same text in all four places;
// tests/test_gpu_world_contacts.py holds the world's lists equal to the
// batch's word for word.
// Device code only.
#pragma once

#include "rb_device.hpp"
#include "rb_boxes.hpp"
#include "rb_internal.hpp"

namespace rb {

// a real into element o of the caller's array
template <typename T> __device__ __forceinline__ void put_real(void *a, int64_t o, T v, bool io32) {
    if (io32) static_cast<float *>(a)[o] = (float)v;
    else static_cast<double *>(a)[o] = (double)v;
}

// slot o of the records.  Q: the query's output arrays (partner, kind, dist,
// pos, frame, io32: ContactQuery, WorldContactQuery)
template <typename T, typename Q>
__device__ __forceinline__ void put_record(const Q &q, int64_t o, int32_t partner, int32_t kind, T dist, V3<T> pos,
                                           V3<T> frame) {
    q.partner[o] = partner;
    q.kind[o] = kind;
    put_real(q.dist, o, dist, q.io32);
    if (q.pos) { put_real(q.pos, 3 * o, pos.x, q.io32); put_real(q.pos, 3 * o + 1, pos.y, q.io32); put_real(q.pos, 3 * o + 2, pos.z, q.io32); }
    if (q.frame) {
        put_real(q.frame, 3 * o, frame.x, q.io32); put_real(q.frame, 3 * o + 1, frame.y, q.io32);
        put_real(q.frame, 3 * o + 2, frame.z, q.io32);
    }
}

// the unused slots [from, R) of the body whose first slot is slot0: kind -1, zeros elsewhere
template <typename T, typename Q>
__device__ __forceinline__ void fill_records(const Q &q, int64_t slot0, int32_t from, int32_t R) {
    const V3<T> zero = {T(0), T(0), T(0)};
    for (int32_t s = from; s < R; ++s) put_record(q, slot0 + s, 0, -1, T(0), zero, zero);
}

// The planes in plane order: a sphere's one contact, a box's corners in bit
// order, at most 4.  plane(a, pn, pp) gives plane a's normal and point;
// emit(partner, kind, contact).  Mi: the box's orientation (kind != 0).
template <typename T, typename Plane, typename Emit>
__device__ __forceinline__ void contacts_planes(int32_t n_planes, Plane plane, int32_t kind, V3<T> x, V3<T> sz,
                                                const M3<T> &Mi, Emit emit) {
    for (int a = 0; a < n_planes; ++a) {
        V3<T> pn, pp;
        plane(a, pn, pp);
        Contact<T> con;
        if (kind == 0) {
            if (plane_sphere(pn, pp, x, sz.x, con)) emit(-1 - a, 0, con);
        } else {
            const V3<T> dif = {x.x - pp.x, x.y - pp.y, x.z - pp.z};
            const T dist = mj_dot(dif, pn);
            int cnt = 0;
            for (int c = 0; c < 8 && cnt < 4; ++c) {
                if (!plane_box_corner(pn, x, dist, Mi, sz, c, con)) continue;
                ++cnt;
                emit(-1 - a, 1 + c, con);
            }
        }
    }
}

// is body b (kind) geom1 of its pair with body j (kind kj)?  The sphere of a
// sphere-box pair, else the lower id: the rule by which contacts_pair orders
// its operands and the step flips the normal (rb_body.hpp solve_sphere_pair,
// rb_batch_body.hpp solve_box_pair).  Those keep the rule inside and hand no
// flag to emit, so the impulse queries (rb_batch_impulses.hip,
// rb_world_impulses.hip) read it here.
__device__ __forceinline__ bool self_is_geom1(int32_t kind, int32_t kj, int b, int j) {
    return (kind == 0 && kj != 0) || ((kind != 0) == (kj != 0) && b < j);
}

// Body b (kind, centre x, half extents sz, bounding radius bi, orientation
// Mi) against body j (kind kj, snapshot sj): two spheres by the step kernels'
// test (sphere_sphere_hit), a box-involved pair (BOXES instances only) by
// overlapping bounding spheres (candidate_hit, rb_step.hpp) and then the
// narrowphase.  geom1: the lower id of two spheres or two boxes, the sphere of
// a sphere-box pair.  ext_j() / quat_j(): body j's half extents and
// orientation, read only for a box-involved pair in range; poly, ps: box_box's
// clipping polygon column in LDS and its stride.  emit(partner, kind, contact).
template <typename T, bool BOXES, typename Ext, typename Quat, typename Emit>
__device__ __forceinline__ void contacts_pair(int32_t b, int32_t j, int32_t kind, int32_t kj, V3<T> x, V3<T> sz, T bi,
                                              const M3<T> &Mi, const Snap<T> &sj, Ext ext_j, Quat quat_j, T *poly,
                                              int ps, Emit emit) {
    const V3<T> cj = {sj.x, sj.y, sj.z};
    if (kind == 0 && kj == 0) {
        if (!sphere_sphere_hit(x, sz.x, cj, sj.r)) return;
        Contact<T> con;
        if (b < j) sphere_sphere(x, sz.x, cj, sj.r, con);      // geom1: the lower id
        else sphere_sphere(cj, sj.r, x, sz.x, con);
        emit(j, 16, con);
        return;
    }
    if constexpr (BOXES) {
        const V3<T> dd = {x.x - cj.x, x.y - cj.y, x.z - cj.z};
        if (!(sqroot(mj_dot(dd, dd)) <= bi + sj.r)) return;
        const V3<T> hj = ext_j();
        M3<T> Mj;
        if (kj != 0) Mj = mj_body_mat(quat_j());
        // (one call of each primitive, operands selected: solve_box_pair, rb_batch_boxes.hip)
        const bool g1 = (kind == 0 && kj != 0) || (kind != 0 && kj != 0 && b < j);
        const V3<T> p1 = g1 ? x : cj, p2 = g1 ? cj : x;
        const V3<T> h1 = g1 ? sz : hj, h2 = g1 ? hj : sz;
        M3<T> M1, M2;
#pragma unroll
        for (int c = 0; c < 9; ++c) { M1.a[c] = g1 ? Mi.a[c] : Mj.a[c]; M2.a[c] = g1 ? Mj.a[c] : Mi.a[c]; }
        if (kind == 0 || kj == 0) {
            Contact<T> con;
            if (sphere_box(p1, g1 ? sz.x : sj.r, p2, M2, h2, con)) emit(j, CK_SPHERE_BOX, con);
        } else {
            box_box(p1, M1, h1, p2, M2, h2, poly, ps, [&](const Contact<T> &c, int ck) { emit(j, ck, c); });
        }
    }
}

}  // namespace rb
