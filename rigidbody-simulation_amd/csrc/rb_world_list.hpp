// rb_world_list.hpp — what the two queries of a world's current state share
// (the contact query, rb_world_contacts.hip; the impulse query,
// rb_world_impulses.hip): a lane's body, its partner list out of the query's
// own table, and the canonical walk over its contacts.
//
// world_list: load once, then the 2 x 2 x 2 neighbourhood of the body's cell
// with the step kernels' one-lane search (rb_grid.hpp search_buckets, a
// partner list of QUERY_MAXP ids kept ascending in the lane's LDS column) and
// their candidate test (rb_step.hpp candidate_hit), and whether the body has
// a list at all.  world_walk: the planes in plane order, then the partners in
// ascending id (rb_contacts.hpp), a partner's data read by id from the state
// rows and the constants.  Neither holds a barrier or writes anything but the
// lane's LDS column and the query's error word (sp.err).
// Device code only.
#pragma once
#include "rb_step.hpp"
#include "rb_contacts.hpp"
#include "rb_world_contacts.hpp"

namespace rb {

static_assert(STEP_BLOCK == 64, "one wave per workgroup: search_buckets strides the LDS columns by STEP_BLOCK");

template <typename T> struct WorldBody {
    int32_t kind;
    V3<T> x, sz;                       // centre; half extents (a sphere: its radius, 0, 0)
    T bi;                              // bounding radius
    Q4<T> qt;                          // orientation (a sphere's: identity unless asked for)
    int32_t np;                        // partners in the lane's column of s_id
    bool listed;                       // the body has a list
};

// Body i of the world behind p (a query's parameter block: WorldContactQuery).
// sphere_q: load a sphere's orientation too (the solve's inertia reads it).
template <typename T, bool BOXES>
__device__ __forceinline__ WorldBody<T> world_list(const StepParams<T> &p, int32_t i, bool sphere_q, int32_t *s_id, int tid) {
    WorldBody<T> b;
    // ---- load once ---------------------------------------------------------
    int32_t kind = 0;
    if constexpr (BOXES) kind = p.cs.kind[i];
    const Snap<T> self = p.snap_cur[i];
    const V3<T> x = {self.x, self.y, self.z};
    const T bi = self.r;
    const V3<T> sz = {p.cs.sx()[i], kind != 0 ? p.cs.sy()[i] : T(0), kind != 0 ? p.cs.sz()[i] : T(0)};
    Q4<T> qt = {T(1), T(0), T(0), T(0)};
    if (kind != 0 || sphere_q) qt = {p.st.qw()[i], p.st.qx()[i], p.st.qy()[i], p.st.qz()[i]};
    // the table's fill overflowed (the insert kernel ran before this one; no
    // lane of this kernel raises that bit): no body of the call has a list
    const bool no_table = (__hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ERR_BUCKET_OVERFLOW) != 0;

    // ---- the partners, ascending id, in the lane's column of s_id ------------
    int32_t cx, cy, cz;
    const bool in_grid = cell_of(x.x, x.y, x.z, p.grid.inv_cs, cx, cy, cz);
    if (!in_grid) atomicOr(p.err, ERR_DOMAIN);
    int32_t np_ = 0, hits = 0;
    if (in_grid && !no_table) {
        bool defer = false;
        // every body is in the table once and every bucket is visited once, so
        // the hits are distinct: more of them than the list holds is an overflow
        // (search_buckets raises ERR_PARTNER_OVERFLOW in sp.err itself)
        np_ = search_buckets<T, QUERY_MAXP, LAYOUT_ANY>(p, i, x, s_id, tid, *p.cur.gen, [&](uint32_t tj, const Snap<T> &s) {
            const bool h = candidate_hit<T, BOXES>(p, i, kind, x, sz.x, bi, tj, s, defer);
            hits += h ? 1 : 0;
            return h;
        });
    }
    b.kind = kind; b.x = x; b.sz = sz; b.bi = bi; b.qt = qt;
    b.np = np_;
    b.listed = in_grid && !no_table && hits <= QUERY_MAXP;
    return b;
}

// The contacts of a listed body i in canonical order: emit(partner, kind,
// contact, self_g1), self_g1: the body is geom1 of the pair (never of a plane
// contact).  poly: box_box's clipping polygon column in LDS (BOXES), stride
// STEP_BLOCK.
template <typename T, bool BOXES, typename Emit>
__device__ __forceinline__ void world_walk(const StepParams<T> &p, int32_t i, const WorldBody<T> &b, const int32_t *s_id,
                                           int tid, T *poly, Emit emit) {
    M3<T> Mi;
    if (b.kind != 0) Mi = mj_body_mat(b.qt);
    contacts_planes<T>(p.n_planes, [&](int a, V3<T> &pn, V3<T> &pp) {
        pn = {p.pn[a][0], p.pn[a][1], p.pn[a][2]};
        pp = {p.pp[a][0], p.pp[a][1], p.pp[a][2]};
    }, b.kind, b.x, b.sz, Mi, [&](int32_t partner, int32_t ck, const Contact<T> &con) { emit(partner, ck, con, false); });
    for (int u = 0; u < b.np; ++u) {
        const int32_t j = s_id[u * STEP_BLOCK + tid];
        int32_t kj = 0;
        if constexpr (BOXES) kj = p.cs.kind[j];
        const bool g1 = self_is_geom1(b.kind, kj, i, j);
        contacts_pair<T, BOXES>(
            i, j, b.kind, kj, b.x, b.sz, b.bi, Mi, p.snap_cur[j],
            [&] { return V3<T>{p.cs.sx()[j], p.cs.sy()[j], p.cs.sz()[j]}; },
            [&] { return Q4<T>{p.st.qw()[j], p.st.qx()[j], p.st.qy()[j], p.st.qz()[j]}; }, poly, STEP_BLOCK,
            [&](int32_t partner, int32_t ck, const Contact<T> &con) { emit(partner, ck, con, g1); });
    }
}

}  // namespace rb
