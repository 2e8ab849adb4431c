// rb_batch_boxes.hip — batched worlds whose template environment mixes
// spheres and boxes (rb_batch_create_mixed): the batch step kernel that holds
// the box narrowphase.
//
// batch_mixed_kernel has the lane mapping, the launch shape (state loaded
// once, up to RB_BATCH_CHUNK steps, stored once, one barrier per step), the
// failure semantics and the frame (rb_batch_frame.hpp) of batch_step_kernel
// (rb_batch.hip).  Beyond it: a lane's kind is the template's kind of its
// body; beside the position snapshots the step-start orientations ping-pong
// in LDS, written by every lane every step (a pair can come into range and
// touch in the same step: DESIGN 2.5); the partners' kinds and half extents
// are put into LDS once per launch; a box-involved pair is a partner when the
// bounding spheres overlap (candidate_hit, rb_step.hpp) and is evaluated by
// solve_box_pair below, body_update's pair block, from step-start data of
// both bodies.  Every other body of the environment is
// visited in ascending id, which is the order of a world's sorted partner
// list, so an environment steps bit-identically to a world of its scene.
//
// The box narrowphase needs more registers than a wave has at two waves per
// SIMD, so the kernel is built as box_kernel is (rb_step.hip): one wave per
// SIMD, register arrays indexed by compile-time constants only, the clipping
// polygon of box_box a column of 48 reals per lane in LDS.
#include "rb_device.hpp"
#include "rb_grid.hpp"
#include "rb_internal.hpp"
#include "rb_body.hpp"
#include "rb_boxes.hpp"
#include "rb_batch_frame.hpp"

namespace rb {

// K2, the box-involved pair of body i (kind, centre x, orientation M, size
// sz) with partner j (kind kj, step-start centre cj, orientation Mj — read
// for a box only —, half extents hj, radius rj where it is a sphere), from
// step-start data of both bodies (rb_boxes.hpp), in MuJoCo's geom order:
// sphere before box, boxes by id.  One contact per emitted point, in
// generation order.  poly, ps: the lane's clipping polygon column in LDS.
// This is the pair block of body_update (rb_step.hpp), a second copy of its
// text: moved into a function that both call, box_kernel's f32 instances
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

// REC: the recording instance of a sampled run
// ENVS: per-environment planes, gravity or applied forces are set
template <typename T, bool REC, bool ENVS>
__global__ __launch_bounds__(BATCH_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1)))
void batch_mixed_kernel(BatchParams<T> p) {
    __shared__ Snap<T> s_snap[2][BATCH_BLOCK];
    __shared__ Q4<T> s_quat[2][BATCH_BLOCK];     // step-start orientations, beside s_snap
    __shared__ T s_ext[3][BATCH_BLOCK];          // half extents (a sphere: its radius, 0, 0)
    __shared__ int32_t s_kind[BATCH_BLOCK];
    __shared__ int32_t s_fail[BATCH_BLOCK];      // per environment of the wave; sticky within a launch
    __shared__ T s_poly[48 * BATCH_BLOCK];       // box-box face clipping: 2 x 8 vertices x 3 per lane

    const int lane = threadIdx.x;
    const int M = p.M;
    const int epw = BATCH_BLOCK / M;             // whole environments per wave
    const int el_raw = lane / M;
    const int b = lane - el_raw * M;             // body within the environment
    // idle lanes (batch_step_kernel) run along on slot 0's data, visit no
    // partner and store nothing
    const bool active = el_raw < epw && (int64_t)blockIdx.x * epw + el_raw < p.E;
    const int el = active ? el_raw : 0;          // environment within the wave
    const int64_t env = (int64_t)blockIdx.x * epw + el;
    const int64_t g = active ? env * M + b : 0;
    const int ebase = el * M;                    // the environment's first lane
    const int nj = active ? M : 0;               // bodies whose pairs this lane evaluates

    // ---- load once ---------------------------------------------------------
    const int32_t kind = p.cs.kind[active ? b : 0];     // [M]: the template's kinds
    const Snap<T> self = p.snap[g];
    V3<T> x = {self.x, self.y, self.z};
    const T bi = self.r;
    Q4<T> q = {p.st.qw()[g], p.st.qx()[g], p.st.qy()[g], p.st.qz()[g]};
    V3<T> v = {p.st.vx()[g], p.st.vy()[g], p.st.vz()[g]};
    V3<T> w = {p.st.wx()[g], p.st.wy()[g], p.st.wz()[g]};
    const T m = p.cs.mass()[g];
    const V3<T> I = {p.cs.ix()[g], p.cs.iy()[g], p.cs.iz()[g]};
    const T sy = p.cs.sy()[g], szz = p.cs.sz()[g];
    const V3<T> sz = {p.cs.sx()[g], kind != 0 ? sy : T(0), kind != 0 ? szz : T(0)};
    const int64_t ev = active ? env : 0;
    // an environment that failed in an earlier launch is not advanced
    bool failed = !active || p.code[ev] != 0;
    int32_t done = 0;

    // the per-step constants solve_contact / apply_force read (rb_body.hpp)
    StepParams<T> sp;
    sp.xfrc = nullptr;
    sp.rec_count = nullptr;
    sp.S = 0;
    batch_consts<T, ENVS>(p, ev, sp);
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
        env_planes_fill(p, blk, lane, epw);          // (visible after the barrier below)
        epl.n_planes = p.n_planes;
        epl.pn = {blk + el, epw};
        epl.pp = {blk + 3 * epw + el, epw};
    }

    // the partners' constants, once per launch
    s_kind[lane] = kind;
    s_ext[0][lane] = sz.x; s_ext[1][lane] = sz.y; s_ext[2][lane] = sz.z;
    s_fail[lane] = 0;
    s_snap[0][lane] = Snap<T>{x.x, x.y, x.z, bi};
    s_quat[0][lane] = q;
    __syncthreads();

    SampleTick tick = {p.phase, p.samp_first};
    T *poly = s_poly + lane;

    for (int s = 0; s < p.k; ++s) {
        const Snap<T> *cur = s_snap[s & 1];
        const Q4<T> *curq = s_quat[s & 1];
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
        M3<T> Mi;                                // box orientation (the narrowphase below needs it too)
        if (kind != 0) Mi = mj_body_mat(q);
        if constexpr (ENVS) {
            if (kind == 0) solve_planes_sphere(sp, epl, 0, x, sz.x, m, kk, invI, vn, wn, nrec);
            else solve_planes_box(sp, epl, 0, x, Mi, sz, m, kk, invI, vn, wn, nrec);
        } else {
            if (kind == 0) solve_planes_sphere(sp, p, 0, x, sz.x, m, kk, invI, vn, wn, nrec);
            else solve_planes_box(sp, p, 0, x, Mi, sz, m, kk, invI, vn, wn, nrec);
        }

        // ---- K2: every other body of the environment, ascending id ----------
        for (int j = 0; j < nj; ++j) {
            if (j == b) continue;
            const Snap<T> sj = cur[ebase + j];
            const V3<T> cj = {sj.x, sj.y, sj.z};
            const int32_t kj = s_kind[ebase + j];
            if (kind == 0 && kj == 0) {
                if (!sphere_sphere_hit(x, sz.x, cj, sj.r)) continue;
                solve_sphere_pair(sp, 0, b, j, x, sz.x, cj, sj.r, m, kk, invI, vn, wn, nrec);
                continue;
            }
            // box-involved: overlapping bounding spheres (candidate_hit, rb_step.hpp)
            const V3<T> dd = {x.x - cj.x, x.y - cj.y, x.z - cj.z};
            if (!(sqroot(mj_dot(dd, dd)) <= bi + sj.r)) continue;
            const V3<T> hj = {s_ext[0][ebase + j], s_ext[1][ebase + j], s_ext[2][ebase + j]};
            M3<T> Mj;
            if (kj != 0) Mj = mj_body_mat(curq[ebase + j]);
            solve_box_pair(sp, 0, b, j, kind, kj, x, Mi, sz, cj, sj.r, Mj, hj, m, kk, invI, vn, wn, nrec, poly,
                           BATCH_BLOCK);
        }

        // ---- K3: integrate (collision.py:90-100) ----------------------------
        V3<T> xn = x;
        Q4<T> qn;
        integrate_pose(xn, qn, q, vn, wn, sp.dt);
        bad = bad || !cell_of(xn.x, xn.y, xn.z, p.inv_cs, cx, cy, cz);

        // a failing body fails its environment: none of its bodies advances
        // (batch_step_kernel)
        if (bad && active) s_fail[el] = 1;
        s_snap[(s + 1) & 1][lane] = Snap<T>{xn.x, xn.y, xn.z, bi};
        s_quat[(s + 1) & 1][lane] = qn;          // every step: the partner of the next step may be new
        __syncthreads();
        failed = failed || s_fail[el] != 0;
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

template <typename T> hipError_t launch_batch_mixed(const BatchParams<T> &p, bool rec, hipStream_t s) {
    if (p.E <= 0 || p.k <= 0) return hipSuccess;
    if (!p.cs.kind || p.M < 2 || p.M > BATCH_BLOCK || p.n_planes < 0 || p.n_planes > MAX_PLANES) return hipErrorInvalidValue;
    if (rec && (!p.samp || p.every < 1 || p.phase < 1 || p.phase > p.every || (p.samp_rows != 7 && p.samp_rows != 13)))
        return hipErrorInvalidValue;
    const int64_t epw = BATCH_BLOCK / p.M;
    const unsigned blocks = (unsigned)((p.E + epw - 1) / epw);
    as_constant(rec, [&](auto REC) {
        as_constant(p.env_planes || p.env_g || p.env_xfrc, [&](auto ENVS) {
            // ENVS: the wave's planes in LDS, [n_planes][6][environments per wave]
            const size_t lds = ENVS.value ? (size_t)epw * (size_t)p.n_planes * 6 * sizeof(T) : 0;
            hipLaunchKernelGGL((batch_mixed_kernel<T, REC.value, ENVS.value>), dim3(blocks), dim3(BATCH_BLOCK), lds, s, p);
        });
    });
    return hipGetLastError();
}

template hipError_t launch_batch_mixed<double>(const BatchParams<double> &, bool, hipStream_t);
template hipError_t launch_batch_mixed<float>(const BatchParams<float> &, bool, hipStream_t);

}  // namespace rb
