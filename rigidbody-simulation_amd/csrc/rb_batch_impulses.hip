// rb_batch_impulses.hip — the impulse query of a batch (rb_batch_impulses.hpp):
// the contact list of the current state, walked in the step's order, with the
// step's solve run on it, and what the solve computes written out instead of
// thrown away: jn and jt of every contact, the body's velocity after gravity,
// applied forces and all its contacts, and its net contact impulse.
//
// One pass, one lane per body, one device body (impulses_body) for both
// mappings: the one-wave mapping of rb_batch_contacts.hip (floor(64 / M) rows
// of the query per workgroup) and the wide mapping of rb_batch_wide.hip (one
// row per workgroup of 128, 192 or 256 threads, lane = body id), each with or
// without a population (the queries keep the fixed E x M mapping for
// populations, as the contact queries do).  A kernel computes its lane mapping
// inline and hands it over by value.
//
// The walk is contacts_planes / contacts_pair (rb_contacts.hpp), so the list,
// its order and the records are the contact query's.  The emit callback is the
// step's treatment of one contact (solve_contact, rb_body.hpp, with jn and jt
// kept): the skip rules, the normal flipped for the geom1 body under
// RB_NORMAL_ORIENTED, impulse / apply (rb_device.hpp) with the step's
// LazyInvI.  Gravity and applied forces are apply_force (rb_body.hpp), by the
// paths batch_step_body takes.  The solve runs over every contact; the record
// bound R cuts records only.
//
// A lane puts what its partners read into LDS once (snapshot; BOXES:
// quaternion, half extents, kind), one barrier, which every lane and every wave
// reaches; nothing returns before it.  All loops are bounded by M, n_planes and
// 8 corners.  The planes come from the parameter block or, where
// rb_batch_set_planes is set, from the environment's rows in global memory
// (one pass reads each once).  The position check of a step is not run: the
// query fails nothing.
//
// BOXES instances are built as batch_contacts_boxes_kernel is: one wave per
// SIMD, register arrays indexed by compile-time constants only, the clipping
// polygon of box_box a column of 48 reals per lane in LDS.  Sphere instances
// hold none of that.
// Built once per real type: RB_INST = 1 fp64, 2 fp32.
#include "rb_device.hpp"
#include "rb_boxes.hpp"
#include "rb_body.hpp"
#include "rb_batch_frame.hpp"
#include "rb_batch_impulses.hpp"
#include "rb_contacts.hpp"
#include "rb_batch_checks.hpp"

namespace rb {
namespace {

// (self_is_geom1, the flag the contact lambda below takes: rb_contacts.hpp)
//
// Lane threadIdx.x of a workgroup of BLOCK threads is body b of the environment
// of row `row` of the query, whose bodies sit in the LDS slots from ebase on;
// in_range: the lane has a row and a body slot (else it loads slot 0's data and
// leaves after the barrier).  BOXES: some body is a box among several; else
// spheres only or (q.c.box) the one box of an M == 1 template.
template <typename T, bool BOXES, int BLOCK>
__device__ __forceinline__ void impulses_body(const BatchParams<T> &p, const Population &pop, const ImpulseQuery &q,
                                              bool in_range, int64_t row_raw, int b, int ebase) {
    __shared__ Snap<T> s_snap[BLOCK];

    const int lane = threadIdx.x;
    const int M = p.M;
    const int64_t row = in_range ? row_raw : 0;
    const int64_t env = !in_range ? 0 : q.c.ids ? q.c.ids[row] : q.c.env0 + row;
    const int ne = pop.n_bodies ? pop.n_bodies[env] : M;      // present bodies: a prefix
    const int64_t g = in_range ? env * M + b : 0;
    const bool present = in_range && b < ne;

    // ---- load once ---------------------------------------------------------
    int32_t kind = q.c.box ? 1 : 0;
    if constexpr (BOXES) kind = pop.kind ? pop.kind[g] : p.cs.kind[in_range ? b : 0];
    const Snap<T> self = p.snap[g];
    const V3<T> x = {self.x, self.y, self.z};
    const T bi = self.r;
    const V3<T> sz = {p.cs.sx()[g], kind != 0 ? p.cs.sy()[g] : T(0), kind != 0 ? p.cs.sz()[g] : T(0)};
    const Q4<T> qt = {p.st.qw()[g], p.st.qx()[g], p.st.qy()[g], p.st.qz()[g]};
    V3<T> v = {p.st.vx()[g], p.st.vy()[g], p.st.vz()[g]};
    V3<T> w = {p.st.wx()[g], p.st.wy()[g], p.st.wz()[g]};
    const T m = p.cs.mass()[g];
    const bool failed = p.code[env] != 0;

    // the per-step constants the law reads (rb_body.hpp), as batch_step_body sets them
    StepParams<T> sp;
    sp.xfrc = nullptr;
    sp.rec_count = nullptr;
    sp.S = 0;
    batch_consts<T, true>(p, env, sp);
    sp.thr = p.thr;
    sp.oriented = p.oriented;

    // what the partners read
    s_snap[lane] = self;
    T *poly = nullptr;
    const Q4<T> *s_q = nullptr;
    const T *s_e = nullptr;
    const int32_t *s_k = nullptr;
    if constexpr (BOXES) {
        __shared__ Q4<T> s_quat[BLOCK];
        __shared__ T s_ext[3 * BLOCK];           // half extents (a sphere: its radius, 0, 0)
        __shared__ int32_t s_kind[BLOCK];
        __shared__ T s_poly[48 * BLOCK];         // box-box face clipping: 2 x 8 vertices x 3 per lane
        s_quat[lane] = qt;
        s_ext[lane] = sz.x; s_ext[BLOCK + lane] = sz.y; s_ext[2 * BLOCK + lane] = sz.z;
        s_kind[lane] = kind;
        poly = s_poly + lane;
        s_q = s_quat; s_e = s_ext; s_k = s_kind;
    }
    __syncthreads();
    if (!in_range) return;

    const bool io32 = q.c.io32;
    const int32_t R = q.c.R;
    const int64_t body = row * M + b;
    const int64_t slot0 = body * (int64_t)R;
    const V3<T> zero = {T(0), T(0), T(0)};
    int32_t n = 0;
    V3<T> net_p = zero, net_l = zero;            // sum of P, sum of r x P, from +0

    if (!failed && present) {
        LazyInvI<T> invI;
        invI.I = {p.cs.ix()[g], p.cs.iy()[g], p.cs.iz()[g]};
        invI.q = qt;
        // ---- a4: gravity; with forces set the applied-force path, all-zero rows included ----
        if (p.env_xfrc) {
            const int64_t N = p.E * M;
            const V3<T> xf = {p.env_xfrc[g], p.env_xfrc[N + g], p.env_xfrc[2 * N + g]};
            const V3<T> xt = {p.env_xfrc[3 * N + g], p.env_xfrc[4 * N + g], p.env_xfrc[5 * N + g]};
            apply_force(sp, m, invI, v, w, xf, xt);
        } else {
            apply_force<T, false>(sp, 0, m, invI, v, w);
        }
        const T kk = impulse_k(m);
        // the inverse inertia once, before the walk (value-identical to the lazy
        // evaluation): each emit site below would else carry the inversion's code,
        // and the instances allocated 27-48 more registers (f64 spheres past 256)
        (void)invI.get();

        // ---- K2 on one contact (solve_contact, rb_body.hpp), jn and jt kept; the record ----
        auto contact = [&](int32_t partner, int32_t ck, const Contact<T> &con, bool self_g1) {
            T jn = T(0);
            V3<T> jt = zero;
            if (con.dist < T(0) && !(absval(con.dist) < sp.thr)) {      // collision.py:74, :79-80
                const V3<T> nn = (sp.oriented && self_g1) ? V3<T>{-con.frame.x, -con.frame.y, -con.frame.z} : con.frame;
                const V3<T> r = {con.pos.x - x.x, con.pos.y - x.y, con.pos.z - x.z};   // :75
                if (impulse(kk, v, w, r, nn, sp.e, sp.mu, jn, jt)) {
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
        };

        // ---- planes, plane order (a plane's frame is never flipped) ----------------
        M3<T> Mi;
        if (kind != 0) Mi = mj_body_mat(qt);
        contacts_planes<T>(p.n_planes, [&](int a, V3<T> &pn, V3<T> &pp) {
            pn = {p.pn[a][0], p.pn[a][1], p.pn[a][2]};
            pp = {p.pp[a][0], p.pp[a][1], p.pp[a][2]};
            if (p.env_planes) {                  // [n_planes][6][E]
                const T *r = p.env_planes + (int64_t)a * 6 * p.E + env;
                pn = {r[0], r[p.E], r[2 * p.E]};
                pp = {r[3 * p.E], r[4 * p.E], r[5 * p.E]};
            }
        }, kind, x, sz, Mi, [&](int32_t partner, int32_t ck, const Contact<T> &con) { contact(partner, ck, con, false); });

        // ---- every other present body of the environment, ascending id -----------
        for (int j = 0; j < ne; ++j) {
            if (j == b) continue;
            const Snap<T> sj = s_snap[ebase + j];
            int32_t kj = kind;                   // (not BOXES: spheres only; the one box has no partner)
            if constexpr (BOXES) kj = s_k[ebase + j];
            const bool g1 = self_is_geom1(kind, kj, b, j);
            contacts_pair<T, BOXES>(b, j, kind, kj, x, sz, bi, Mi, sj,
                                    [&]() { return V3<T>{s_e[ebase + j], s_e[BLOCK + ebase + j], s_e[2 * BLOCK + ebase + j]}; },
                                    [&]() { return s_q[ebase + j]; }, poly, BLOCK,
                                    [&](int32_t partner, int32_t ck, const Contact<T> &con) { contact(partner, ck, con, g1); });
        }
    } else {
        v = zero;                                // a failed environment, an absent body: rows of zeros
        w = zero;
    }

    // ---- the count (an absent body: 0), the unused slots, the body's rows -----------
    q.c.counts[body] = failed ? -1 : n;
    for (int32_t s = n < R ? n : R; s < R; ++s) {
        const int64_t o = slot0 + s;
        put_record(q.c, o, 0, -1, T(0), zero, zero);
        put_real(q.jn, o, T(0), io32);
        put_real(q.jt, 3 * o, T(0), io32); put_real(q.jt, 3 * o + 1, T(0), io32); put_real(q.jt, 3 * o + 2, T(0), io32);
    }
    if (q.vel) {
        const int64_t o = 6 * body;
        put_real(q.vel, o, v.x, io32); put_real(q.vel, o + 1, v.y, io32); put_real(q.vel, o + 2, v.z, io32);
        put_real(q.vel, o + 3, w.x, io32); put_real(q.vel, o + 4, w.y, io32); put_real(q.vel, o + 5, w.z, io32);
    }
    if (q.net) {
        const int64_t o = 6 * body;
        put_real(q.net, o, net_p.x, io32); put_real(q.net, o + 1, net_p.y, io32); put_real(q.net, o + 2, net_p.z, io32);
        put_real(q.net, o + 3, net_l.x, io32); put_real(q.net, o + 4, net_l.y, io32); put_real(q.net, o + 5, net_l.z, io32);
    }
}

// M <= 64: floor(64 / M) rows of the query per one-wave workgroup (rb_batch_contacts.hip)
template <typename T, bool BOXES>
__global__ __launch_bounds__(BATCH_BLOCK) __attribute__((amdgpu_waves_per_eu(BOXES ? 1 : 2, BOXES ? 1 : 8)))
void batch_impulses_kernel(BatchParams<T> p, Population pop, ImpulseQuery q) {
    const int lane = threadIdx.x;
    const int M = p.M;
    const int epw = BATCH_BLOCK / M;             // whole environments (rows) per wave
    const int el = lane / M;
    const int64_t row = (int64_t)blockIdx.x * epw + el;
    // lanes past the wave's last whole environment, or past the query, are idle
    const bool in_range = el < epw && row < q.c.n;
    impulses_body<T, BOXES, BATCH_BLOCK>(p, pop, q, in_range, row, lane - el * M, in_range ? el * M : 0);
}

// 65..256 bodies: one row per workgroup, lane = body id (rb_batch_wide.hip)
template <typename T, bool BOXES, int BLOCK>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(BOXES ? 1 : 2, BOXES ? 1 : 8)))
void batch_impulses_wide_kernel(BatchParams<T> p, Population pop, ImpulseQuery q) {
    static_assert(BLOCK % 64 == 0 && BLOCK > BATCH_BLOCK && BLOCK <= BATCH_WIDE_MAX, "one lane per body, whole waves");
    const int lane = threadIdx.x;
    const bool in_range = lane < p.M;            // (the grid is q.c.n workgroups)
    impulses_body<T, BOXES, BLOCK>(p, pop, q, in_range, blockIdx.x, in_range ? lane : 0, 0);
}

}  // namespace

template <typename T>
hipError_t launch_batch_impulses(const BatchParams<T> &p, const Population &pop, const ImpulseQuery &q, bool boxes,
                                 hipStream_t s) {
    if (q.c.n <= 0) return hipSuccess;
    if (!query_ok(p, q.c, 1, BATCH_WIDE_MAX) || q.c.pos || q.c.frame) return hipErrorInvalidValue;
    if (q.c.R > 0 && (!q.jn || !q.jt)) return hipErrorInvalidValue;
    // the kinds of a BOXES instance: the population's, else the template's (a mixed template holds two bodies or more)
    if (boxes ? !(pop.kind || (p.cs.kind && p.M >= 2)) : q.c.box && p.M != 1) return hipErrorInvalidValue;
    as_constant(boxes, [&](auto BOXES) {
        if (p.M > BATCH_BLOCK) {
            with_block(p.M, [&](auto BLOCK) {
                hipLaunchKernelGGL((batch_impulses_wide_kernel<T, BOXES.value, BLOCK.value>), dim3((unsigned)q.c.n),
                                   dim3(BLOCK.value), 0, s, p, pop, q);
            });
        } else {
            const int64_t epw = BATCH_BLOCK / p.M;
            const unsigned blocks = (unsigned)((q.c.n + epw - 1) / epw);
            hipLaunchKernelGGL((batch_impulses_kernel<T, BOXES.value>), dim3(blocks), dim3(BATCH_BLOCK), 0, s, p, pop, q);
        }
    });
    return hipGetLastError();
}

#if RB_INST == 1
using Real = double;
#elif RB_INST == 2
using Real = float;
#else
#error "RB_INST: 1 (fp64) or 2 (fp32)"
#endif
template hipError_t launch_batch_impulses<Real>(const BatchParams<Real> &, const Population &, const ImpulseQuery &, bool,
                                                hipStream_t);

}  // namespace rb
