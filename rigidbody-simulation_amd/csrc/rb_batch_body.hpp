// rb_batch_body.hpp — what the batch step kernels with a pair loop share
// (rb_batch_boxes.hip, rb_batch_wide.hip, rb_batch_ragged.hip): the
// box-involved pair of a step (solve_box_pair, one copy for the three units)
// and the step of a lane of any mapping (batch_step_body: batch_wide_kernel,
// ragged_step_kernel, ragged_wide_kernel).  A kernel computes its lane mapping
// (which environment, which body, where the environment's lanes begin, how
// many partners, its kind) inline and hands it over by value; everything from
// "load once" to batch_finish is here, once.
// Not on the body: batch_step_kernel and batch_balls_kernel (rb_batch.hip),
// and batch_mixed_kernel (rb_batch_boxes.hip), which on the body measured
// 0.5 % slower on a 4-body pile and keeps its text (DESIGN 4.3,
// profiles/batch_unify).
#pragma once

#include <type_traits>
#include "rb_device.hpp"
#include "rb_grid.hpp"
#include "rb_internal.hpp"
#include "rb_body.hpp"
#include "rb_boxes.hpp"
#include "rb_batch_frame.hpp"
#include "rb_batch_checks.hpp"

namespace rb {

// K2, the box-involved pair of body i (kind, centre x, orientation M, size
// sz) with partner j (kind kj, step-start centre cj, orientation Mj — read
// for a box only —, half extents hj, radius rj where it is a sphere), from
// step-start data of both bodies (rb_boxes.hpp), in MuJoCo's geom order:
// sphere before box, boxes by id.  One contact per emitted point, in
// generation order.  poly, ps: the lane's clipping polygon column in LDS.
// This is the pair block of body_update (rb_step.hpp), the batch's copy of
// its text: moved into a function that both call, box_kernel's f32 instances
// allocated 247 registers instead of 249, and body_update's
// code is pinned.
template <typename T>
__device__ __forceinline__ void solve_box_pair(const StepParams<T> &p, int32_t l, int32_t i, int32_t j, int32_t kind,
                                               int32_t kj, V3<T> x, const M3<T> &M, V3<T> sz, V3<T> cj, T rj,
                                               const M3<T> &Mj, V3<T> hj, T m, T k, LazyInvI<T> &invI, V3<T> &v,
                                               V3<T> &w, int32_t &nrec, T *poly, int ps) {
    auto emit = [&](const Contact<T> &con, int ck, bool self_g1) {
        record(p, l, nrec, j, ck, con.dist);
        const V3<T> n = (p.oriented && self_g1) ? V3<T>{-con.frame.x, -con.frame.y, -con.frame.z} : con.frame;
        solve_contact(p, con, x, n, m, k, invI, v, w);
    };
    // geom1: the sphere of a sphere-box pair, else the lower id
    // (one call of each primitive, operands selected)
    const bool g1 = (kind == 0 && kj != 0) || (kind != 0 && kj != 0 && i < j);
    const V3<T> p1 = g1 ? x : cj, p2 = g1 ? cj : x;
    const V3<T> h1 = g1 ? sz : hj, h2 = g1 ? hj : sz;
    M3<T> M1, M2;
#pragma unroll
    for (int c = 0; c < 9; ++c) { M1.a[c] = g1 ? M.a[c] : Mj.a[c]; M2.a[c] = g1 ? Mj.a[c] : M.a[c]; }
    if (kind == 0 || kj == 0) {
        Contact<T> con;
        if (sphere_box(p1, g1 ? sz.x : rj, p2, M2, h2, con)) emit(con, CK_SPHERE_BOX, g1);
    } else {
        box_box(p1, M1, h1, p2, M2, h2, poly, ps, [&](const Contact<T> &c, int ck) { emit(c, ck, g1); });
    }
}

// A launch of a batch step kernel from a lane's point of view: state loaded
// once, up to RB_BATCH_CHUNK steps with one barrier each, stored once.  Lane
// threadIdx.x of a workgroup of BLOCK threads is body b of environment env,
// row g = env * M + b of the batch; the environment's bodies sit in the LDS
// slots from ebase on, and the lane evaluates its pairs with bodies 0..nj-1 in
// ascending id, which is the order of a world's sorted partner list, so an
// environment steps bit-identically to a world of its present bodies.  An idle
// lane (!active) runs along on whatever valid row the caller gives it, has
// nj == 0, fails nothing, stores nothing, and reaches every barrier: nothing
// returns before the step loop ends.
//
// BOXES: some body is a box (kind: this lane's); else spheres only: no
//        polygon, orientation, extent or kind LDS.  Beside the position
//        snapshots the step-start orientations ping-pong in LDS, written by
//        every lane every step (a pair can come into range and touch in the
//        same step: DESIGN 2.5); the partners' kinds and half extents go into
//        LDS once per launch; a box-involved pair is a partner when the
//        bounding spheres overlap (candidate_hit, rb_step.hpp).
// REC:   the recording instance of a sampled run.
// ENVS:  per-environment planes, gravity or applied forces may be set: the
//        planes come from the block's dynamic LDS, [plane][component][stride],
//        which fill(blk) fills, column el being this lane's environment's;
//        gravity and forces are tested at run time.  Else the template's.
// The failure flag: in a one-wave block slot el, the environment's, sticky
// within the launch.  Across waves it ping-pongs as the snapshots do, since
// waves leave a barrier at different times: step s raises and reads word
// s & 1, which nobody writes again before the barrier of step s + 1; a word
// is never cleared: once it is read as set every lane is failed for good.
template <typename T, bool BOXES, bool REC, bool ENVS, int BLOCK, typename Fill>
__device__ __forceinline__ void batch_step_body(const BatchParams<T> &p, bool active, int64_t g, int64_t env, int b,
                                                int ebase, int nj, int32_t kind, int el, int stride, Fill fill) {
    constexpr bool WAVES = BLOCK > BATCH_BLOCK;  // the environment spans several waves
    __shared__ Snap<T> s_snap[2][BLOCK];
    __shared__ int32_t s_fail[WAVES ? 2 : BLOCK];

    const int lane = threadIdx.x;
    const int M = p.M;

    // ---- load once ---------------------------------------------------------
    const Snap<T> self = p.snap[g];
    V3<T> x = {self.x, self.y, self.z};
    const T bi = self.r;
    Q4<T> q = {p.st.qw()[g], p.st.qx()[g], p.st.qy()[g], p.st.qz()[g]};
    V3<T> v = {p.st.vx()[g], p.st.vy()[g], p.st.vz()[g]};
    V3<T> w = {p.st.wx()[g], p.st.wy()[g], p.st.wz()[g]};
    const T m = p.cs.mass()[g];
    const V3<T> I = {p.cs.ix()[g], p.cs.iy()[g], p.cs.iz()[g]};
    V3<T> sz = {p.cs.sx()[g], T(0), T(0)};
    if constexpr (BOXES) {
        const T sy = p.cs.sy()[g], szz = p.cs.sz()[g];
        sz = {sz.x, kind != 0 ? sy : T(0), kind != 0 ? szz : T(0)};
    }
    // an environment that failed in an earlier launch is not advanced
    bool failed = !active || p.code[env] != 0;
    int32_t done = 0;

    // the per-step constants solve_contact / apply_force read (rb_body.hpp)
    StepParams<T> sp;
    sp.xfrc = nullptr;
    sp.rec_count = nullptr;
    sp.S = 0;
    batch_consts<T, ENVS>(p, env, sp);
    sp.thr = p.thr;
    sp.oriented = p.oriented;

    // ---- ENVS: the environment's planes, the body's applied force -----------
    V3<T> xf = {T(0), T(0), T(0)}, xt = xf;
    EnvPlanes<T> epl{};
    if constexpr (ENVS) {
        if (p.env_xfrc) {
            const int64_t N = p.E * M;
            xf = {p.env_xfrc[g], p.env_xfrc[N + g], p.env_xfrc[2 * N + g]};
            xt = {p.env_xfrc[3 * N + g], p.env_xfrc[4 * N + g], p.env_xfrc[5 * N + g]};
        }
        T *blk = reinterpret_cast<T *>(s_env_dyn);
        fill(blk);                                   // (visible after the barrier below)
        epl.n_planes = p.n_planes;
        epl.pn = {blk + el, stride};
        epl.pp = {blk + 3 * stride + el, stride};
    }

    // the partners' constants, once per launch
    T *poly = nullptr;
    const Q4<T> *s_q = nullptr;
    Q4<T> *s_qw = nullptr;
    const T *s_e = nullptr;
    const int32_t *s_k = nullptr;
    if constexpr (BOXES) {
        __shared__ Q4<T> s_quat[2 * BLOCK];      // step-start orientations, beside s_snap: [2][BLOCK]
        __shared__ T s_ext[3 * BLOCK];           // half extents (a sphere: its radius, 0, 0): [3][BLOCK]
        __shared__ int32_t s_kind[BLOCK];
        __shared__ T s_poly[48 * BLOCK];         // box-box face clipping: 2 x 8 vertices x 3 per lane
        s_kind[lane] = kind;
        s_ext[lane] = sz.x; s_ext[BLOCK + lane] = sz.y; s_ext[2 * BLOCK + lane] = sz.z;
        s_quat[lane] = q;
        poly = s_poly + lane;
        s_q = s_quat; s_qw = s_quat; s_e = s_ext; s_k = s_kind;
    }
    if (!WAVES || lane < 2) s_fail[lane] = 0;
    s_snap[0][lane] = Snap<T>{x.x, x.y, x.z, bi};
    __syncthreads();

    SampleTick tick = {p.phase, p.samp_first};

    for (int s = 0; s < p.k; ++s) {
        const Snap<T> *cur = s_snap[s & 1];
        int32_t cx, cy, cz;
        bool bad = !cell_of(x.x, x.y, x.z, p.inv_cs, cx, cy, cz);     // the step-start position

        V3<T> vn = v, wn = w;
        LazyInvI<T> invI;
        invI.I = I;
        invI.q = q;
        // ---- a4: gravity; ENVS with forces set: the applied-force path ---------
        if (ENVS && p.env_xfrc) apply_force(sp, m, invI, vn, wn, xf, xt);
        else apply_force<T, false>(sp, 0, m, invI, vn, wn);
        const T kk = impulse_k(m);

        // ---- K2: plane contacts, plane order, by the lane's kind ---------------
        int32_t nrec = 0;                        // (sp.rec_count is null: nothing is recorded)
        [[maybe_unused]] M3<T> Mi;               // box orientation (the narrowphase below needs it too)
        auto planes = [&](const auto &pl) {      // pl: the block's planes (ENVS) or the template's
            if constexpr (BOXES) {
                if (kind != 0) Mi = mj_body_mat(q);
                if (kind == 0) solve_planes_sphere(sp, pl, 0, x, sz.x, m, kk, invI, vn, wn, nrec);
                else solve_planes_box(sp, pl, 0, x, Mi, sz, m, kk, invI, vn, wn, nrec);
            } else {
                solve_planes_sphere(sp, pl, 0, x, sz.x, m, kk, invI, vn, wn, nrec);
            }
        };
        if constexpr (ENVS) planes(epl);
        else planes(p);

        // ---- K2: every other body of the environment, ascending id ----------
        // (planes and pair as lambdas: what they declare ends with the call, and
        // the kernels allocate fewer registers than with the same text in line)
        auto pair = [&](int j) {
            const Snap<T> sj = cur[ebase + j];
            const V3<T> cj = {sj.x, sj.y, sj.z};
            int32_t kj = 0;
            if constexpr (BOXES) kj = s_k[ebase + j];
            if (kind == 0 && kj == 0) {
                if (!sphere_sphere_hit(x, sz.x, cj, sj.r)) return;
                solve_sphere_pair(sp, 0, b, j, x, sz.x, cj, sj.r, m, kk, invI, vn, wn, nrec);
                return;
            }
            if constexpr (BOXES) {
                // box-involved: overlapping bounding spheres (candidate_hit, rb_step.hpp)
                const V3<T> dd = {x.x - cj.x, x.y - cj.y, x.z - cj.z};
                if (!(sqroot(mj_dot(dd, dd)) <= bi + sj.r)) return;
                const V3<T> hj = {s_e[ebase + j], s_e[BLOCK + ebase + j], s_e[2 * BLOCK + ebase + j]};
                M3<T> Mj;
                if (kj != 0) Mj = mj_body_mat(s_q[(s & 1) * BLOCK + ebase + j]);
                solve_box_pair(sp, 0, b, j, kind, kj, x, Mi, sz, cj, sj.r, Mj, hj, m, kk, invI, vn, wn, nrec, poly, BLOCK);
            }
        };
        for (int j = 0; j < nj; ++j)
            if (j != b) pair(j);

        // ---- K3: integrate (collision.py:90-100) ----------------------------
        V3<T> xn = x;
        Q4<T> qn;
        integrate_pose(xn, qn, q, vn, wn, sp.dt);
        bad = bad || !cell_of(xn.x, xn.y, xn.z, p.inv_cs, cx, cy, cz);

        // a failing body fails its environment: none of its bodies advances, in any wave
        const int fw = WAVES ? s & 1 : el;
        if (bad && active) s_fail[fw] = 1;
        s_snap[(s + 1) & 1][lane] = Snap<T>{xn.x, xn.y, xn.z, bi};
        if constexpr (BOXES) s_qw[((s + 1) & 1) * BLOCK + lane] = qn;   // every step: the partner of the next step may be new
        __syncthreads();
        failed = failed || s_fail[fw] != 0;
        if (!failed) {
            x = xn; q = qn; v = vn; w = wn;
            ++done;
        }
        if constexpr (REC) sample_tick(p, tick, active, g, x, q, v, w);
    }

    // ---- store once ------------------------------------------------------------
    if (!active) return;
    if (done > 0) {
        p.snap[g] = Snap<T>{x.x, x.y, x.z, bi};
        p.st.qw()[g] = q.w; p.st.qx()[g] = q.x; p.st.qy()[g] = q.y; p.st.qz()[g] = q.z;
        p.st.vx()[g] = v.x; p.st.vy()[g] = v.y; p.st.vz()[g] = v.z;
        p.st.wx()[g] = w.x; p.st.wy()[g] = w.y; p.st.wz()[g] = w.z;
    }
    batch_finish(p, b, env, done);
}

}  // namespace rb
