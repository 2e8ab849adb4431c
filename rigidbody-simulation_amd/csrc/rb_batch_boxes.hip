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
// solve_box_pair (rb_batch_body.hpp), body_update's pair block, from
// step-start data of both bodies.  Every other body of the environment is
// visited in ascending id, which is the order of a world's sorted partner
// list, so an environment steps bit-identically to a world of its scene.
//
// The box narrowphase needs more registers than a wave has at two waves per
// SIMD, so the kernel is built as box_kernel is (rb_step.hip): one wave per
// SIMD, register arrays indexed by compile-time constants only, the clipping
// polygon of box_box a column of 48 reals per lane in LDS.
//
// The step below is the text batch_step_body (rb_batch_body.hpp) was made
// from.  This kernel alone stays off it: on the body its instances kept
// registers and LDS, and a pile of 4 bodies ran 0.5 % slower in all three
// processes of the A/B (cause not found; DESIGN 4.3, profiles/batch_unify).
// A change to the step sequence is made there and here.
#include "rb_batch_body.hpp"

namespace rb {

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
    if (rec && !rec_ok(p)) return hipErrorInvalidValue;
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
