// rb_batch_sensed.hip — the sensing step loop of a sampled run
// (rb_batch_sensed.hpp): batch_step_body's launch (state loaded once, up to
// RB_BATCH_CHUNK steps in registers with one barrier each, stored once, the
// failure flag and the sample tick) with the contacts of a step walked as the
// impulse query walks them (contacts_planes / contacts_pair, rb_contacts.hpp;
// contact_impulse, rb_impulse_contact.hpp), so that what a step's solve computes
// is there to keep: the body's net contact impulse of the step.  A committed
// step adds it to the window's sum; a sample tick stores the sum beside the
// state rows that were asked for and starts the next window from +0.  The sum
// of a window that a launch leaves open goes to the batch's carry rows
// (SensedRun::acc) at the launch's end and comes back at the next one's start.
//
// One device body (sensed_body) for both mappings, which are the queries': the
// fixed E x M mapping, a population honoured through n_bodies and kind.  A lane
// that holds no present body, and every lane of an environment that has
// failed, skips the step's work and still reaches the step's barrier; nothing
// returns before the step loop ends.  All inner loops are bounded by M,
// n_planes and 8 corners.
//
// The planes of the workgroup's environments are put into dynamic LDS once per
// launch (env_planes_fill, rb_batch_frame.hpp: the environment's rows, or the
// template's planes), so a step reads its planes one way and never from global
// memory.  BOXES instances are built as batch_impulses_kernel's are: one wave
// per SIMD, the clipping polygon a column of 48 reals per lane in LDS; beside
// the position snapshots the step-start orientations ping-pong, kinds and half
// extents are written once per launch.  Sphere instances hold none of that.
// Built once per real type: RB_INST = 1 fp64, 2 fp32.
#include "rb_device.hpp"
#include "rb_grid.hpp"
#include "rb_boxes.hpp"
#include "rb_body.hpp"
#include "rb_batch_frame.hpp"
#include "rb_batch_sensed.hpp"
#include "rb_impulse_contact.hpp"
#include "rb_contacts.hpp"
#include "rb_batch_checks.hpp"

namespace rb {
namespace {

// Lane threadIdx.x of a workgroup of BLOCK threads is body b of environment
// env_raw, whose bodies sit in the LDS slots from ebase on and whose planes are
// column el of the block's epw; in_range: the lane has an environment and a
// body slot (else it runs along on row 0, steps nothing and stores nothing).
template <typename T, bool BOXES, int BLOCK>
__device__ __forceinline__ void sensed_body(const BatchParams<T> &p, const Population &pop, const SensedRun &r,
                                            bool in_range, int64_t env_raw, int b, int ebase, int el, int epw) {
    constexpr bool WAVES = BLOCK > BATCH_BLOCK;  // the environment spans several waves
    __shared__ Snap<T> s_snap[2][BLOCK];
    __shared__ int32_t s_fail[WAVES ? 2 : BLOCK];

    const int lane = threadIdx.x;
    const int M = p.M;
    const int64_t N = p.E * M;
    const int64_t env = in_range ? env_raw : 0;
    const int ne = pop.n_bodies ? pop.n_bodies[env] : M;      // present bodies: a prefix
    const int64_t g = in_range ? env * M + b : 0;
    const bool present = in_range && b < ne;

    // ---- load once ---------------------------------------------------------
    int32_t kind = r.box ? 1 : 0;
    if constexpr (BOXES) kind = pop.kind ? pop.kind[g] : p.cs.kind[in_range ? b : 0];
    const Snap<T> self = p.snap[g];
    V3<T> x = {self.x, self.y, self.z};
    const T bi = self.r;
    Q4<T> q = {p.st.qw()[g], p.st.qx()[g], p.st.qy()[g], p.st.qz()[g]};
    V3<T> v = {p.st.vx()[g], p.st.vy()[g], p.st.vz()[g]};
    V3<T> w = {p.st.wx()[g], p.st.wy()[g], p.st.wz()[g]};
    const T m = p.cs.mass()[g];
    const V3<T> I = {p.cs.ix()[g], p.cs.iy()[g], p.cs.iz()[g]};
    const V3<T> sz = {p.cs.sx()[g], kind != 0 ? p.cs.sy()[g] : T(0), kind != 0 ? p.cs.sz()[g] : T(0)};
    // an environment that failed in an earlier launch is not advanced
    bool failed = !present || p.code[env] != 0;
    int32_t done = 0;

    // the per-step constants the law reads (rb_body.hpp), as batch_step_body sets them
    StepParams<T> sp;
    sp.xfrc = nullptr;
    sp.rec_count = nullptr;
    sp.S = 0;
    batch_consts<T, true>(p, env, sp);
    sp.thr = p.thr;
    sp.oriented = p.oriented;

    // the body's applied force; the window's sum so far (sum of P, sum of r x P)
    const V3<T> zero = {T(0), T(0), T(0)};
    V3<T> xf = zero, xt = zero;
    if (p.env_xfrc) {
        xf = {p.env_xfrc[g], p.env_xfrc[N + g], p.env_xfrc[2 * N + g]};
        xt = {p.env_xfrc[3 * N + g], p.env_xfrc[4 * N + g], p.env_xfrc[5 * N + g]};
    }
    T *acc = static_cast<T *>(r.acc);
    V3<T> win_p = zero, win_l = zero;
    if (present) {
        win_p = {acc[g], acc[N + g], acc[2 * N + g]};
        win_l = {acc[3 * N + g], acc[4 * N + g], acc[5 * N + g]};
    }

    // the planes of the block's environments, [plane][component][epw] (visible after the barrier below)
    T *blk = reinterpret_cast<T *>(s_env_dyn);
    env_planes_fill(p, blk, lane, epw);

    // the partners' constants, once per launch
    T *poly = nullptr;
    Q4<T> *s_q = nullptr;
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
        s_q = s_quat; s_e = s_ext; s_k = s_kind;
    }
    if (!WAVES || lane < 2) s_fail[lane] = 0;
    s_snap[0][lane] = self;
    __syncthreads();

    SampleTick tick = {p.phase, p.samp_first};

    for (int s = 0; s < p.k; ++s) {
        const Snap<T> *cur = s_snap[s & 1];
        bool bad = false;
        V3<T> xn = x, vn = v, wn = w;
        Q4<T> qn = q;
        V3<T> net_p = zero, net_l = zero;        // the step's sum of P, of r x P, from +0

        if (!failed) {
            int32_t cx, cy, cz;
            bad = !cell_of(x.x, x.y, x.z, p.inv_cs, cx, cy, cz);      // the step-start position
            LazyInvI<T> invI;
            invI.I = I;
            invI.q = q;
            // ---- a4: gravity; with forces set the applied-force path, all-zero rows included ----
            if (p.env_xfrc) apply_force(sp, m, invI, vn, wn, xf, xt);
            else apply_force<T, false>(sp, 0, m, invI, vn, wn);
            const T kk = impulse_k(m);
            (void)invI.get();                    // once, before the walk (impulses_body, rb_batch_impulses.hip)

            auto contact = [&](const Contact<T> &con, bool self_g1) {
                T jn = T(0);
                V3<T> jt = zero;
                contact_impulse(sp, con, self_g1, x, m, kk, invI, vn, wn, jn, jt, net_p, net_l);
            };

            // ---- planes, plane order (a plane's frame is never flipped) ----------------
            M3<T> Mi;
            if (kind != 0) Mi = mj_body_mat(q);
            contacts_planes<T>(p.n_planes, [&](int a, V3<T> &pn, V3<T> &pp) {
                const T *c = blk + a * 6 * epw + el;
                pn = {c[0], c[epw], c[2 * epw]};
                pp = {c[3 * epw], c[4 * epw], c[5 * epw]};
            }, kind, x, sz, Mi, [&](int32_t, int32_t, const Contact<T> &con) { contact(con, false); });

            // ---- every other present body of the environment, ascending id -----------
            for (int j = 0; j < ne; ++j) {
                if (j == b) continue;
                const Snap<T> sj = cur[ebase + j];
                int32_t kj = kind;               // (not BOXES: spheres only; the one box has no partner)
                if constexpr (BOXES) kj = s_k[ebase + j];
                const bool g1 = self_is_geom1(kind, kj, b, j);
                contacts_pair<T, BOXES>(b, j, kind, kj, x, sz, bi, Mi, sj,
                                        [&]() { return V3<T>{s_e[ebase + j], s_e[BLOCK + ebase + j], s_e[2 * BLOCK + ebase + j]}; },
                                        [&]() { return s_q[(s & 1) * BLOCK + ebase + j]; }, poly, BLOCK,
                                        [&](int32_t, int32_t, const Contact<T> &con) { contact(con, g1); });
            }

            // ---- K3: integrate (collision.py:90-100) ----------------------------
            integrate_pose(xn, qn, q, vn, wn, sp.dt);
            bad = bad || !cell_of(xn.x, xn.y, xn.z, p.inv_cs, cx, cy, cz);
        }

        // a failing body fails its environment: none of its bodies advances, in any wave
        const int fw = WAVES ? s & 1 : el;
        if (bad) s_fail[fw] = 1;
        s_snap[(s + 1) & 1][lane] = Snap<T>{xn.x, xn.y, xn.z, bi};
        if constexpr (BOXES) s_q[((s + 1) & 1) * BLOCK + lane] = qn;
        __syncthreads();
        failed = failed || s_fail[fw] != 0;
        if (!failed) {
            x = xn; q = qn; v = vn; w = wn;
            ++done;
            // a committed step's row joins the window, component by component
            win_p = {win_p.x + net_p.x, win_p.y + net_p.y, win_p.z + net_p.z};
            win_l = {win_l.x + net_l.x, win_l.y + net_l.y, win_l.z + net_l.z};
        }

        // ---- the sample tick: the rows asked for and the window's sum; the next window ----
        if (--tick.until == 0) {
            if (present && tick.slot >= 0 && tick.slot < p.samp_slots) {
                T *o = p.samp + (int64_t)tick.slot * p.samp_rows * N + g;
                if (r.row_q >= 0) {
                    T *oq = o + r.row_q * N;
                    oq[0] = x.x; oq[N] = x.y; oq[2 * N] = x.z;
                    oq[3 * N] = q.w; oq[4 * N] = q.x; oq[5 * N] = q.y; oq[6 * N] = q.z;
                }
                if (r.row_v >= 0) {
                    T *ov = o + r.row_v * N;
                    ov[0] = v.x; ov[N] = v.y; ov[2 * N] = v.z;
                    ov[3 * N] = w.x; ov[4 * N] = w.y; ov[5 * N] = w.z;
                }
                T *on = o + r.row_net * N;
                on[0] = win_p.x; on[N] = win_p.y; on[2 * N] = win_p.z;
                on[3 * N] = win_l.x; on[4 * N] = win_l.y; on[5 * N] = win_l.z;
            }
            ++tick.slot;
            tick.until = p.every;
            win_p = zero;
            win_l = zero;
        }
    }

    // ---- store once ------------------------------------------------------------
    if (!present) return;
    if (done > 0) {
        p.snap[g] = Snap<T>{x.x, x.y, x.z, bi};
        p.st.qw()[g] = q.w; p.st.qx()[g] = q.x; p.st.qy()[g] = q.y; p.st.qz()[g] = q.z;
        p.st.vx()[g] = v.x; p.st.vy()[g] = v.y; p.st.vz()[g] = v.z;
        p.st.wx()[g] = w.x; p.st.wy()[g] = w.y; p.st.wz()[g] = w.z;
    }
    acc[g] = win_p.x; acc[N + g] = win_p.y; acc[2 * N + g] = win_p.z;
    acc[3 * N + g] = win_l.x; acc[4 * N + g] = win_l.y; acc[5 * N + g] = win_l.z;
    batch_finish(p, b, env, done);
}

// M <= 64: floor(64 / M) environments per one-wave workgroup
template <typename T, bool BOXES>
__global__ __launch_bounds__(BATCH_BLOCK) __attribute__((amdgpu_waves_per_eu(BOXES ? 1 : 2, BOXES ? 1 : 8)))
void sensed_run_kernel(BatchParams<T> p, Population pop, SensedRun r) {
    const int lane = threadIdx.x;
    const int M = p.M;
    const int epw = BATCH_BLOCK / M;             // whole environments per wave
    const int el = lane / M;
    const int64_t env = (int64_t)blockIdx.x * epw + el;
    // lanes past the wave's last whole environment, or past the batch, are idle
    const bool in_range = el < epw && env < p.E;
    sensed_body<T, BOXES, BATCH_BLOCK>(p, pop, r, in_range, env, lane - el * M, in_range ? el * M : 0, in_range ? el : 0, epw);
}

// 65..256 bodies: one environment per workgroup, lane = body id
template <typename T, bool BOXES, int BLOCK>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(BOXES ? 1 : 2, BOXES ? 1 : 8)))
void sensed_run_wide_kernel(BatchParams<T> p, Population pop, SensedRun r) {
    static_assert(BLOCK % 64 == 0 && BLOCK > BATCH_BLOCK && BLOCK <= BATCH_WIDE_MAX, "one lane per body, whole waves");
    const int lane = threadIdx.x;
    const bool in_range = lane < p.M;            // (the grid is p.E workgroups)
    sensed_body<T, BOXES, BLOCK>(p, pop, r, in_range, blockIdx.x, in_range ? lane : 0, 0, 0, 1);
}

// slot i / N, body i % N of the drained slots -> the caller's rows
template <typename T, typename IO>
__global__ __launch_bounds__(256) void sensed_out_kernel(const T *samp, int64_t total, int32_t rows, SensedRun r, int64_t N,
                                                         IO *qpos, IO *qvel, IO *net) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const T *o = samp + (i / N) * rows * N + i % N;
    if (qpos)
        for (int c = 0; c < 7; ++c) qpos[7 * i + c] = (IO)o[(r.row_q + c) * N];
    if (qvel)
        for (int c = 0; c < 6; ++c) qvel[6 * i + c] = (IO)o[(r.row_v + c) * N];
    for (int c = 0; c < 6; ++c) net[6 * i + c] = (IO)o[(r.row_net + c) * N];
}

}  // namespace

template <typename T>
hipError_t launch_batch_sensed(const BatchParams<T> &p, const Population &pop, const SensedRun &r, bool boxes, hipStream_t s) {
    if (p.E <= 0) return hipSuccess;
    if (p.M < 1 || p.M > BATCH_WIDE_MAX || p.n_planes < 0 || p.n_planes > MAX_PLANES || p.k < 1 || p.k > BATCH_CHUNK)
        return hipErrorInvalidValue;
    // the schedule (a launch without a sample: phase past its steps) and the slots' rows
    if (!p.samp || !r.acc || p.every < 1 || p.phase < 1 || p.samp_first < 0 || p.samp_slots < 1) return hipErrorInvalidValue;
    if (r.row_net < 0 || p.samp_rows != r.row_net + 6 || r.row_q >= r.row_net || r.row_v >= r.row_net) return hipErrorInvalidValue;
    // the kinds of a BOXES instance: the population's, else the template's (a mixed template holds two bodies or more)
    if (boxes ? !(pop.kind || (p.cs.kind && p.M >= 2)) : r.box && p.M != 1) return hipErrorInvalidValue;
    as_constant(boxes, [&](auto BOXES) {
        if (p.M > BATCH_BLOCK) {
            const size_t lds = (size_t)p.n_planes * 6 * sizeof(T);
            with_block(p.M, [&](auto BLOCK) {
                hipLaunchKernelGGL((sensed_run_wide_kernel<T, BOXES.value, BLOCK.value>), dim3((unsigned)p.E), dim3(BLOCK.value),
                                   lds, s, p, pop, r);
            });
        } else {
            const int64_t epw = BATCH_BLOCK / p.M;
            const unsigned blocks = (unsigned)((p.E + epw - 1) / epw);
            const size_t lds = (size_t)epw * (size_t)p.n_planes * 6 * sizeof(T);
            hipLaunchKernelGGL((sensed_run_kernel<T, BOXES.value>), dim3(blocks), dim3(BATCH_BLOCK), lds, s, p, pop, r);
        }
    });
    return hipGetLastError();
}

template <typename T, typename IO>
hipError_t launch_sensed_out(const T *samp, int32_t n, int32_t rows, const SensedRun &r, int64_t N, IO *qpos, IO *qvel,
                             IO *net, hipStream_t s) {
    if (n <= 0 || N <= 0) return hipSuccess;
    if (!samp || !net || r.row_net < 0 || rows != r.row_net + 6) return hipErrorInvalidValue;
    if ((qpos && r.row_q < 0) || (qvel && r.row_v < 0)) return hipErrorInvalidValue;
    const int64_t total = (int64_t)n * N;
    hipLaunchKernelGGL((sensed_out_kernel<T, IO>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, samp, total, rows, r,
                       N, qpos, qvel, net);
    return hipGetLastError();
}

#if RB_INST == 1
using Real = double;
#elif RB_INST == 2
using Real = float;
#else
#error "RB_INST: 1 (fp64) or 2 (fp32)"
#endif
template hipError_t launch_batch_sensed<Real>(const BatchParams<Real> &, const Population &, const SensedRun &, bool,
                                              hipStream_t);
template hipError_t launch_sensed_out<Real, double>(const Real *, int32_t, int32_t, const SensedRun &, int64_t, double *,
                                                    double *, double *, hipStream_t);
template hipError_t launch_sensed_out<Real, float>(const Real *, int32_t, int32_t, const SensedRun &, int64_t, float *,
                                                   float *, float *, hipStream_t);

}  // namespace rb
