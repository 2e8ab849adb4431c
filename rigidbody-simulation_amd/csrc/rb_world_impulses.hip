// rb_world_impulses.hip — the impulse query of a world (rb_world_impulses.hpp):
// the contact query's list of the current state, walked in the step's order,
// with the step's solve run on it and what the solve computes written out: jn
// and jt of every contact, the body's velocity after gravity, applied forces
// and all its contacts, and its net contact impulse.
//
// One lane per queried body, one wave per workgroup.  The first half is the
// contact query's (rb_world_list.hpp world_list: load once, the one-lane search
// of the query's own table into the lane's LDS column, the `listed` decision);
// the second half is the solve of the batch's query (rb_batch_impulses.hip
// impulses_body): apply_force as body_update calls it (the world's xfrc, stride
// S, all-zero rows included once forces are set), impulse_k, the inverse
// inertia once before the walk, then world_walk with the step's treatment of
// one contact as its emit: the skip rules, the normal flipped for the geom1
// body under RB_NORMAL_ORIENTED, impulse / apply (rb_device.hpp), the net sums.
// The solve runs over every contact; the record bound R cuts records only.
//
// Nothing of the world is written; a lane without a list stores QUERY_NO_LIST,
// unused slots and rows of zeros.  No barrier; plain vector stores; no atomic
// but world_list's ERR_DOMAIN bit in the query's own error word.  Loops are
// bounded by the list length (QUERY_MAXP), n_planes and 8 corners.
//
// Two instances per real type, as the contact query's: spheres only, and the
// one with the box narrowphase (one wave per SIMD, the clipping polygon a
// column of 48 reals per lane in LDS).
// Built once per real type: RB_INST = 1 fp64, 2 fp32.
#include "rb_world_list.hpp"
#include "rb_world_impulses.hpp"

namespace rb {
namespace {

template <typename T, bool BOXES>
__device__ __forceinline__ void world_impulses_body(const WorldImpulseQuery<T> &q) {
    __shared__ int32_t s_id[QUERY_MAXP * STEP_BLOCK];

    const int tid = threadIdx.x;
    const int64_t k = (int64_t)blockIdx.x * STEP_BLOCK + tid;
    if (k >= q.c.count) return;                  // (no barrier below: lanes past the range store nothing)
    const StepParams<T> &p = q.c.sp;
    const int32_t i = (int32_t)(q.c.first + k);  // (one rank: the body's row of the state and of xfrc is its id)
    T *poly = nullptr;
    if constexpr (BOXES) {
        __shared__ T s_poly[48 * STEP_BLOCK];    // box-box face clipping: 2 x 8 vertices x 3 per lane
        poly = s_poly + tid;
    }
    const WorldBody<T> b = world_list<T, BOXES>(p, i, true, s_id, tid);

    const bool io32 = q.c.io32;
    const int32_t R = q.c.R;
    const int64_t slot0 = k * (int64_t)R;
    const V3<T> zero = {T(0), T(0), T(0)};
    const V3<T> x = b.x;
    int32_t n = 0;
    V3<T> v = zero, w = zero;                    // a body without a list: rows of zeros
    V3<T> net_p = zero, net_l = zero;            // sum of P, sum of r x P, from +0

    if (b.listed) {
        v = {p.st.vx()[i], p.st.vy()[i], p.st.vz()[i]};
        w = {p.st.wx()[i], p.st.wy()[i], p.st.wz()[i]};
        const T m = p.cs.mass()[i];
        LazyInvI<T> invI;
        invI.I = {p.cs.ix()[i], p.cs.iy()[i], p.cs.iz()[i]};
        invI.q = b.qt;
        // ---- a4: gravity; with forces set the applied-force path, all-zero rows included ----
        apply_force(p, i, m, invI, v, w);
        const T kk = impulse_k(m);
        // (the inverse inertia once, before the walk: value-identical to the lazy
        // evaluation, and no emit site carries the inversion's code)
        (void)invI.get();

        // ---- K2 on one contact (solve_contact, rb_body.hpp), jn and jt kept; the record ----
        world_walk<T, BOXES>(p, i, b, s_id, tid, poly, [&](int32_t partner, int32_t ck, const Contact<T> &con, bool self_g1) {
            T jn = T(0);
            V3<T> jt = zero;
            if (con.dist < T(0) && !(absval(con.dist) < p.thr)) {       // collision.py:74, :79-80
                const V3<T> nn = (p.oriented && self_g1) ? V3<T>{-con.frame.x, -con.frame.y, -con.frame.z} : con.frame;
                const V3<T> r = {con.pos.x - x.x, con.pos.y - x.y, con.pos.z - x.z};   // :75
                if (impulse(kk, v, w, r, nn, p.e, p.mu, jn, jt)) {
                    apply(v, w, m, invI.get(), r, nn, jn, jt);
                    const V3<T> P = {jn * nn.x + jt.x, jn * nn.y + jt.y, jn * nn.z + jt.z};   // (as apply evaluates it)
                    const V3<T> L = np_cross(r, P);
                    net_p = {net_p.x + P.x, net_p.y + P.y, net_p.z + P.z};
                    net_l = {net_l.x + L.x, net_l.y + L.y, net_l.z + L.z};
                }
            }
            if (n < R) {
                const int64_t o = slot0 + n;
                put_record(q.c, o, partner, ck, con.dist, zero, zero);
                put_real(q.jn, o, jn, io32);
                put_real(q.jt, 3 * o, jt.x, io32); put_real(q.jt, 3 * o + 1, jt.y, io32); put_real(q.jt, 3 * o + 2, jt.z, io32);
            }
            ++n;
        });
    }

    // ---- the count, the unused slots, the body's rows ------------------------------
    q.c.counts[k] = b.listed ? n : QUERY_NO_LIST;
    for (int32_t s = n < R ? n : R; s < R; ++s) {
        const int64_t o = slot0 + s;
        put_record(q.c, o, 0, -1, T(0), zero, zero);
        put_real(q.jn, o, T(0), io32);
        put_real(q.jt, 3 * o, T(0), io32); put_real(q.jt, 3 * o + 1, T(0), io32); put_real(q.jt, 3 * o + 2, T(0), io32);
    }
    if (q.vel) {
        const int64_t o = 6 * k;
        put_real(q.vel, o, v.x, io32); put_real(q.vel, o + 1, v.y, io32); put_real(q.vel, o + 2, v.z, io32);
        put_real(q.vel, o + 3, w.x, io32); put_real(q.vel, o + 4, w.y, io32); put_real(q.vel, o + 5, w.z, io32);
    }
    if (q.net) {
        const int64_t o = 6 * k;
        put_real(q.net, o, net_p.x, io32); put_real(q.net, o + 1, net_p.y, io32); put_real(q.net, o + 2, net_p.z, io32);
        put_real(q.net, o + 3, net_l.x, io32); put_real(q.net, o + 4, net_l.y, io32); put_real(q.net, o + 5, net_l.z, io32);
    }
}

template <typename T>
__global__ __launch_bounds__(STEP_BLOCK) void world_impulses_kernel(WorldImpulseQuery<T> q) {
    world_impulses_body<T, false>(q);
}

template <typename T>
__global__ __launch_bounds__(STEP_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1)))
void world_impulses_boxes_kernel(WorldImpulseQuery<T> q) {
    world_impulses_body<T, true>(q);
}

}  // namespace

template <typename T> hipError_t launch_world_impulses(const WorldImpulseQuery<T> &q, bool boxes, hipStream_t s) {
    const WorldContactQuery<T> &c = q.c;
    if (c.count <= 0) return hipSuccess;
    const StepParams<T> &p = c.sp;
    if (c.first < 0 || c.first + c.count > p.n_global || p.n_global > INT32_MAX || c.R < 0 || !c.counts)
        return hipErrorInvalidValue;
    if (c.R > 0 && (!c.partner || !c.kind || !c.dist || !q.jn || !q.jt)) return hipErrorInvalidValue;
    if (c.pos || c.frame) return hipErrorInvalidValue;
    if (!p.snap_cur || !p.st.base || !p.cs.base || !p.cur.line || !p.cur.gen || !p.err || p.next.line) return hipErrorInvalidValue;
    if (p.n_planes < 0 || p.n_planes > MAX_PLANES || p.grid.H <= 0 || (boxes && !p.cs.kind)) return hipErrorInvalidValue;
    if (p.n_local != p.n_global || p.lo != 0 || p.S < p.n_global) return hipErrorInvalidValue;   // (one rank: row == id)
    const unsigned blocks = (unsigned)((c.count + STEP_BLOCK - 1) / STEP_BLOCK);
    if (boxes) hipLaunchKernelGGL((world_impulses_boxes_kernel<T>), dim3(blocks), dim3(STEP_BLOCK), 0, s, q);
    else hipLaunchKernelGGL((world_impulses_kernel<T>), dim3(blocks), dim3(STEP_BLOCK), 0, s, q);
    return hipGetLastError();
}

#if RB_INST == 1
using Real = double;
#elif RB_INST == 2
using Real = float;
#else
#error "RB_INST: 1 (fp64) or 2 (fp32)"
#endif
template hipError_t launch_world_impulses<Real>(const WorldImpulseQuery<Real> &, bool, hipStream_t);

}  // namespace rb
