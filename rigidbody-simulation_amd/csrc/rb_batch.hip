// rb_batch.hip — batched worlds: many small independent scenes (environments)
// of M <= 64 bodies each, stepped by one launch (rb_batch_* in include/rbhip.h).
//
// Body b of environment e is global slot g = e * M + b; state and constants
// are struct-of-arrays rows of length E * M.  One lane per body, a wave
// (= one 64-thread workgroup) holds floor(64 / M) whole environments, so an
// environment never spans two waves and all synchronisation is wave-level.
//
// No broadphase: the partners of a body are found by testing every other
// body of its own environment (at most 63) against the step-start snapshots,
// which ping-pong in LDS.  A launch loads the 13 state values and the
// constants of a body once, runs up to RB_BATCH_CHUNK steps in registers and
// stores once.  Each step is body_update's sequence (rb_step.hpp) built
// from the same functions (rb_body.hpp, rb_device.hpp), so an environment
// steps bit-identically to a world of the same scene.  The two-ball law
// (batch_balls_kernel) has the same shape; the law itself, pair evaluation
// included, is in rb_balls.hpp, as for the world's kernels.  The two step
// kernels share a frame (step constants, sampling tick, epilogue:
// rb_batch_frame.hpp) with the kernel of box-involved pairs (rb_batch_boxes.hip).
//
// Sampled runs (rb_batch_run_sampled) launch the recording instances (REC):
// inside the register loop, after every every-th step of the run, a lane
// stores its committed state into a slot of the sample buffer, laid out as
// the state rows are (rows of E * M reals per slot: a wave's stores are
// contiguous); batch_samples_out_kernel turns slots into the boundary's rows.
#include <type_traits>
#include "rb_device.hpp"
#include "rb_grid.hpp"
#include "rb_internal.hpp"
#include "rb_body.hpp"
#include "rb_balls.hpp"
#include "rb_batch_frame.hpp"

namespace rb {

// BOX: the template environment is one box (M == 1); else spheres only
// REC: the recording instance of a sampled run
// ENVS: per-environment planes, gravity or applied forces are set (each of
// the three optional: a null pointer means the batch's)
template <typename T, bool BOX, bool REC, bool ENVS>
__global__ __launch_bounds__(BATCH_BLOCK) void batch_step_kernel(BatchParams<T> p) {
    __shared__ Snap<T> s_snap[2][BATCH_BLOCK];
    __shared__ int32_t s_fail[BATCH_BLOCK];      // per environment of the wave; sticky within a launch

    const int lane = threadIdx.x;
    const int M = p.M;
    const int epw = BATCH_BLOCK / M;             // whole environments per wave
    const int el_raw = lane / M;
    const int b = lane - el_raw * M;             // body within the environment
    // lanes past the wave's last whole environment, or past the batch, are
    // idle: they run along on slot 0's data and store nothing
    const bool active = el_raw < epw && (int64_t)blockIdx.x * epw + el_raw < p.E;
    const int el = active ? el_raw : 0;          // environment within the wave
    const int64_t env = (int64_t)blockIdx.x * epw + el;
    const int64_t g = active ? env * M + b : 0;
    const int ebase = el * M;                    // the environment's first lane

    // ---- load once ---------------------------------------------------------
    const Snap<T> self = p.snap[g];
    V3<T> x = {self.x, self.y, self.z};
    const T bi = self.r;
    Q4<T> q = {p.st.qw()[g], p.st.qx()[g], p.st.qy()[g], p.st.qz()[g]};
    V3<T> v = {p.st.vx()[g], p.st.vy()[g], p.st.vz()[g]};
    V3<T> w = {p.st.wx()[g], p.st.wy()[g], p.st.wz()[g]};
    const T m = p.cs.mass()[g];
    const V3<T> I = {p.cs.ix()[g], p.cs.iy()[g], p.cs.iz()[g]};
    const V3<T> sz = {p.cs.sx()[g], BOX ? p.cs.sy()[g] : T(0), BOX ? p.cs.sz()[g] : T(0)};
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

    s_fail[lane] = 0;
    s_snap[0][lane] = Snap<T>{x.x, x.y, x.z, bi};
    __syncthreads();

    SampleTick tick = {p.phase, p.samp_first};

    for (int s = 0; s < p.k; ++s) {
        const Snap<T> *cur = s_snap[s & 1];
        Snap<T> *nxt = s_snap[(s + 1) & 1];
        int32_t cx, cy, cz;
        bool bad = !cell_of(x.x, x.y, x.z, p.inv_cs, cx, cy, cz);     // the step-start position

        V3<T> vn = v, wn = w;
        LazyInvI<T> invI;
        invI.I = I;
        invI.q = q;
        // ---- a4: gravity (collision.py:66-70); ENVS with forces set: every
        // body takes the applied-force path, all-zero rows included ----------
        if (ENVS && p.env_xfrc) apply_force(sp, m, invI, vn, wn, xf, xt);
        else apply_force<T, false>(sp, 0, m, invI, vn, wn);
        const T kk = impulse_k(m);

        // ---- K2: plane contacts, plane order (the planes: the batch's, or
        // ENVS: the environment's, from LDS) ----------------------------------
        int32_t nrec = 0;                        // (sp.rec_count is null: nothing is recorded)
        if constexpr (ENVS) {
            if constexpr (!BOX) solve_planes_sphere(sp, epl, 0, x, sz.x, m, kk, invI, vn, wn, nrec);
            else solve_planes_box(sp, epl, 0, x, mj_body_mat(q), sz, m, kk, invI, vn, wn, nrec);
        } else {
            if constexpr (!BOX) solve_planes_sphere(sp, p, 0, x, sz.x, m, kk, invI, vn, wn, nrec);
            else solve_planes_box(sp, p, 0, x, mj_body_mat(q), sz, m, kk, invI, vn, wn, nrec);
        }

        // ---- K2: every other body of the environment, ascending id ----------
        if constexpr (!BOX) {
            for (int j = 0; j < M; ++j) {
                if (j == b) continue;
                const Snap<T> sj = cur[ebase + j];
                const V3<T> cj = {sj.x, sj.y, sj.z};
                if (!sphere_sphere_hit(x, sz.x, cj, sj.r)) continue;
                solve_sphere_pair(sp, 0, b, j, x, sz.x, cj, sj.r, m, kk, invI, vn, wn, nrec);
            }
        }

        // ---- K3: integrate (collision.py:90-100) ----------------------------
        V3<T> xn = x;
        Q4<T> qn;
        integrate_pose(xn, qn, q, vn, wn, sp.dt);
        bad = bad || !cell_of(xn.x, xn.y, xn.z, p.inv_cs, cx, cy, cz);

        // a failing body fails its environment: none of its bodies advances
        // (the snapshots a failed environment leaves in LDS are read by its
        // own lanes only, which commit nothing from then on)
        if (bad && active) s_fail[el] = 1;
        nxt[lane] = Snap<T>{xn.x, xn.y, xn.z, bi};
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


// The two-ball law (ball_collision.py:73-125; every expression of it is in
// rb_balls.hpp) with the lane and environment mapping and the frame of
// batch_step_kernel.  The registers hold a ball's true state (x, v, w) and the post-ground state of the coming step (gx, gv, gw:
// gravity and the ground contact depend on the ball alone), which is what the
// partners read from LDS: positions and radius in Snap, velocity and spin in
// Vel, both ping-pong, so a step has one barrier.  A step evaluates every
// pair (a < b) within reach from the post-ground state of both balls and
// accumulates this ball's deltas in ascending partner id (ball_body,
// rb_balls.hip, without grid or partner list), integrates, and runs the next
// step's ground phase.  Nothing survives a launch but the true state: the
// first ground phase is run from it, so dt, e and mu may change between calls.
// The quaternion is never touched (REC loads it to record it).
// ENVS: per-environment gravity is set (the law takes neither per-environment
// planes nor applied forces)
template <typename T, bool REC, bool ENVS>
__global__ __launch_bounds__(BATCH_BLOCK) void batch_balls_kernel(BatchParams<T> p) {
    __shared__ Snap<T> s_snap[2][BATCH_BLOCK];
    __shared__ Vel<T> s_vel[2][BATCH_BLOCK];
    __shared__ T s_mass[BATCH_BLOCK];
    __shared__ int32_t s_fail[BATCH_BLOCK];      // per environment of the wave; sticky within a launch

    const int lane = threadIdx.x;
    const int M = p.M;
    const int epw = BATCH_BLOCK / M;
    const int el_raw = lane / M;
    const int b = lane - el_raw * M;
    const bool active = el_raw < epw && (int64_t)blockIdx.x * epw + el_raw < p.E;   // (idle lanes: batch_step_kernel)
    const int el = active ? el_raw : 0;
    const int64_t env = (int64_t)blockIdx.x * epw + el;
    const int64_t g = active ? env * M + b : 0;
    const int ebase = el * M;

    // ---- load once ---------------------------------------------------------
    const Snap<T> self = p.snap[g];
    V3<T> x = {self.x, self.y, self.z};
    const T ri = self.r;
    V3<T> v = {p.st.vx()[g], p.st.vy()[g], p.st.vz()[g]};
    V3<T> w = {p.st.wx()[g], p.st.wy()[g], p.st.wz()[g]};
    Q4<T> q = {T(1), T(0), T(0), T(0)};
    if constexpr (REC) q = {p.st.qw()[g], p.st.qx()[g], p.st.qy()[g], p.st.qz()[g]};
    const T mi = p.cs.mass()[g];
    const M3<T> Ii = ball_iinv(mi, ri);          // ball_collision.py:39-41 (the inertia rows are not read)
    const int64_t ev = active ? env : 0;
    bool failed = !active || p.code[ev] != 0;
    int32_t done = 0;

    // the constants ball_ground and ball_pair read
    StepParams<T> sp;
    sp.ground = p.ground;
    batch_consts<T, ENVS>(p, ev, sp);
    const T tol = p.tol;

    // the first step's ground phase, from the true state
    V3<T> gx = x, gv = v, gw = w;
    ball_ground(sp, gx, gv, gw, mi, ri, Ii);
    s_fail[lane] = 0;
    s_mass[lane] = mi;
    s_snap[0][lane] = Snap<T>{gx.x, gx.y, gx.z, ri};
    s_vel[0][lane] = Vel<T>{gv.x, gv.y, gv.z, gw.x, gw.y, gw.z, T(0), T(0)};
    __syncthreads();

    SampleTick tick = {p.phase, p.samp_first};

    for (int s = 0; s < p.k; ++s) {
        const Snap<T> *cur = s_snap[s & 1];
        const Vel<T> *curv = s_vel[s & 1];
        int32_t cx, cy, cz;
        // the positions a world under this law checks: the post-ground ones
        bool bad = !cell_of(gx.x, gx.y, gx.z, p.inv_cs, cx, cy, cz);

        // ---- every other ball of the environment, ascending id ---------------
        // (ball_pair, rb_balls.hpp; the partner's Vel and mass are read on a hit only)
        const V3<T> xo = gx, vo = gv, wo = gw;
        V3<T> xa = xo, va = vo, wa = wo;
        for (int j = 0; j < M; ++j) {
            if (j == b) continue;
            const Snap<T> sj = cur[ebase + j];
            const V3<T> xj = {sj.x, sj.y, sj.z};
            const bool self_a = b < j;
            if (!(self_a ? ball_hit(xo, ri, xj, sj.r, tol) : ball_hit(xj, sj.r, xo, ri, tol))) continue;
            const Vel<T> vj = curv[ebase + j];
            ball_pair(xo, vo, wo, mi, ri, Ii, xj, V3<T>{vj.vx, vj.vy, vj.vz}, V3<T>{vj.wx, vj.wy, vj.wz},
                      s_mass[ebase + j], sj.r, self_a, sp.e, sp.mu, tol, xa, va, wa);
        }

        // ---- integrate (:121-122): the true end-of-step state ------------------
        const V3<T> xn = {xa.x + va.x * sp.dt, xa.y + va.y * sp.dt, xa.z + va.z * sp.dt};

        // ---- the next step's ground phase ------------------------------------
        V3<T> ngx = xn, ngv = va, ngw = wa;
        ball_ground(sp, ngx, ngv, ngw, mi, ri, Ii);
        bad = bad || !cell_of(ngx.x, ngx.y, ngx.z, p.inv_cs, cx, cy, cz);

        // a failing ball fails its environment (batch_step_kernel)
        if (bad && active) s_fail[el] = 1;
        s_snap[(s + 1) & 1][lane] = Snap<T>{ngx.x, ngx.y, ngx.z, ri};
        s_vel[(s + 1) & 1][lane] = Vel<T>{ngv.x, ngv.y, ngv.z, ngw.x, ngw.y, ngw.z, T(0), T(0)};
        __syncthreads();
        failed = failed || s_fail[el] != 0;
        if (!failed) {
            x = xn; v = va; w = wa;
            gx = ngx; gv = ngv; gw = ngw;
            ++done;
        }
        if constexpr (REC) sample_tick(p, tick, active, g, x, q, v, w);
    }

    // ---- store once ------------------------------------------------------------
    if (!active) return;
    if (done > 0) {
        p.snap[g] = Snap<T>{x.x, x.y, x.z, ri};
        p.st.vx()[g] = v.x; p.st.vy()[g] = v.y; p.st.vz()[g] = v.z;
        p.st.wx()[g] = w.x; p.st.wy()[g] = w.y; p.st.wz()[g] = w.z;
    }
    batch_finish(p, b, env, done);
}

// Slots [first, first + n) of the sample buffer into the boundary's rows (the
// layout of rb_batch_get_state, a block of [E * M] rows per sample), in double.
template <typename T>
__global__ __launch_bounds__(256) void batch_samples_out_kernel(const T *samp, int32_t first, int64_t total, int32_t rows,
                                                                int64_t N, double *qpos, double *qvel) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int64_t k = t / N, g = t - k * N;
    const T *in = samp + (first + k) * rows * N + g;
    double *q = qpos + 7 * t;
#pragma unroll
    for (int d = 0; d < 7; ++d) q[d] = (double)in[d * N];
    if (rows == 13) {
        double *v = qvel + 6 * t;
#pragma unroll
        for (int d = 0; d < 6; ++d) v[d] = (double)in[(7 + d) * N];
    }
}

// rb_batch_set_state / rb_batch_get_state for a list of environments: row t
// of the caller's arrays is body t % M of environment ids[t / M].  (All
// environments in order: state_in_kernel / state_out_kernel, rb_io.hip.)
template <typename T>
__global__ __launch_bounds__(256) void batch_state_in_kernel(StateIO<T> p, const int64_t *ids, int64_t rows, int32_t M) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows) return;
    const int64_t g = ids[t / M] * M + t % M;
    const double *q = p.qpos + 7 * t, *v = p.qvel + 6 * t;
    p.snap[g] = Snap<T>{(T)q[0], (T)q[1], (T)q[2], p.bound[g]};
#pragma unroll
    for (int d = 0; d < 4; ++d) p.st.row(d)[g] = (T)q[3 + d];
#pragma unroll
    for (int d = 0; d < 6; ++d) p.st.row(4 + d)[g] = (T)v[d];
#pragma unroll
    for (int d = 0; d < 3; ++d) p.st.row(10 + d)[g] = (T)q[d];
}

template <typename T>
__global__ __launch_bounds__(256) void batch_state_out_kernel(StateIO<T> p, const int64_t *ids, int64_t rows, int32_t M) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows) return;
    const int64_t g = ids[t / M] * M + t % M;
    double *q = p.qpos + 7 * t, *v = p.qvel + 6 * t;
    const Snap<T> s = p.snap[g];
    q[0] = (double)s.x; q[1] = (double)s.y; q[2] = (double)s.z;
#pragma unroll
    for (int d = 0; d < 4; ++d) q[3 + d] = (double)p.st.row(d)[g];
#pragma unroll
    for (int d = 0; d < 6; ++d) v[d] = (double)p.st.row(4 + d)[g];
}

// a per-environment reset (rb_batch_set_state): status and step count of the
// listed environments (ids == nullptr: the first n)
__global__ __launch_bounds__(256) void batch_reset_kernel(int32_t *code, int64_t *steps_done, const int64_t *ids, int64_t n) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int64_t e = ids ? ids[t] : t;
    code[e] = 0;
    steps_done[e] = 0;
}

__global__ __launch_bounds__(256) void batch_count_kernel(const int32_t *code, int64_t E, int32_t *out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E && code[e] != 0) atomicAdd(out, 1);
}

// new bounding radii (rb_batch_set_bodies) into the snapshots
template <typename T> __global__ __launch_bounds__(256) void batch_bound_kernel(Snap<T> *snap, const T *bound, int64_t N) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < N) snap[g].r = bound[g];
}

static unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

template <typename T> hipError_t launch_batch_step(const BatchParams<T> &p, bool box, bool balls, bool rec, hipStream_t s) {
    if (p.E <= 0 || p.k <= 0) return hipSuccess;
    if (balls && box) return hipErrorInvalidValue;
    if (p.M < 1 || p.M > BATCH_BLOCK || p.n_planes < 0 || p.n_planes > MAX_PLANES) return hipErrorInvalidValue;
    if (rec && (!p.samp || p.every < 1 || p.phase < 1 || p.phase > p.every || (p.samp_rows != 7 && p.samp_rows != 13)))
        return hipErrorInvalidValue;
    const int64_t epw = BATCH_BLOCK / p.M;
    const unsigned blocks = (unsigned)((p.E + epw - 1) / epw);
    const dim3 gr(blocks), bl(BATCH_BLOCK);
    // the ENVS instances: only with a per-environment array set
    if (balls) {
        if (p.env_planes || p.env_xfrc) return hipErrorInvalidValue;    // (refused by the setters under this law)
        as_constant(rec, [&](auto REC) {
            as_constant(p.env_g != nullptr, [&](auto ENVS) {
                hipLaunchKernelGGL((batch_balls_kernel<T, REC.value, ENVS.value>), gr, bl, 0, s, p);
            });
        });
    } else {
        as_constant(box, [&](auto BOX) {
            as_constant(rec, [&](auto REC) {
                as_constant(p.env_planes || p.env_g || p.env_xfrc, [&](auto ENVS) {
                    // ENVS: the wave's planes in LDS, [n_planes][6][environments per wave]
                    const size_t lds = ENVS.value ? (size_t)epw * (size_t)p.n_planes * 6 * sizeof(T) : 0;
                    hipLaunchKernelGGL((batch_step_kernel<T, BOX.value, REC.value, ENVS.value>), gr, bl, lds, s, p);
                });
            });
        });
    }
    return hipGetLastError();
}
template <typename T>
hipError_t launch_batch_samples_out(const T *samp, int32_t first, int32_t n, int32_t rows, int64_t N, double *qpos,
                                    double *qvel, hipStream_t s) {
    if (n <= 0 || N <= 0) return hipSuccess;
    if (!samp || !qpos || first < 0 || (rows != 7 && rows != 13) || (rows == 13 && !qvel)) return hipErrorInvalidValue;
    const int64_t total = (int64_t)n * N;
    hipLaunchKernelGGL((batch_samples_out_kernel<T>), dim3(blocks256(total)), dim3(256), 0, s, samp, first, total, rows, N,
                       qpos, qvel);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_batch_state_in(const StateIO<T> &p, const int64_t *ids, int64_t n, int32_t M, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((batch_state_in_kernel<T>), dim3(blocks256(n * M)), dim3(256), 0, s, p, ids, n * M, M);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_batch_state_out(const StateIO<T> &p, const int64_t *ids, int64_t n, int32_t M, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((batch_state_out_kernel<T>), dim3(blocks256(n * M)), dim3(256), 0, s, p, ids, n * M, M);
    return hipGetLastError();
}
hipError_t launch_batch_reset(int32_t *code, int64_t *steps_done, const int64_t *ids, int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(batch_reset_kernel, dim3(blocks256(n)), dim3(256), 0, s, code, steps_done, ids, n);
    return hipGetLastError();
}
hipError_t launch_batch_count(const int32_t *code, int64_t E, int32_t *out, hipStream_t s) {
    hipLaunchKernelGGL(batch_count_kernel, dim3(blocks256(E)), dim3(256), 0, s, code, E, out);
    return hipGetLastError();
}
template <typename T> hipError_t launch_batch_bound(Snap<T> *snap, const T *bound, int64_t N, hipStream_t s) {
    hipLaunchKernelGGL((batch_bound_kernel<T>), dim3(blocks256(N)), dim3(256), 0, s, snap, bound, N);
    return hipGetLastError();
}

template hipError_t launch_batch_step<double>(const BatchParams<double> &, bool, bool, bool, hipStream_t);
template hipError_t launch_batch_step<float>(const BatchParams<float> &, bool, bool, bool, hipStream_t);
template hipError_t launch_batch_samples_out<double>(const double *, int32_t, int32_t, int32_t, int64_t, double *, double *,
                                                     hipStream_t);
template hipError_t launch_batch_samples_out<float>(const float *, int32_t, int32_t, int32_t, int64_t, double *, double *,
                                                    hipStream_t);
template hipError_t launch_batch_state_in<double>(const StateIO<double> &, const int64_t *, int64_t, int32_t, hipStream_t);
template hipError_t launch_batch_state_in<float>(const StateIO<float> &, const int64_t *, int64_t, int32_t, hipStream_t);
template hipError_t launch_batch_state_out<double>(const StateIO<double> &, const int64_t *, int64_t, int32_t, hipStream_t);
template hipError_t launch_batch_state_out<float>(const StateIO<float> &, const int64_t *, int64_t, int32_t, hipStream_t);
template hipError_t launch_batch_bound<double>(Snap<double> *, const double *, int64_t, hipStream_t);
template hipError_t launch_batch_bound<float>(Snap<float> *, const float *, int64_t, hipStream_t);

}  // namespace rb
