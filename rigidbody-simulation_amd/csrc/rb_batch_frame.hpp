// rb_batch_frame.hpp — the frame the batch step kernels share (rb_batch.hip:
// batch_step_kernel, batch_balls_kernel; rb_batch_boxes.hip:
// batch_mixed_kernel; rb_batch_body.hpp: batch_step_body): the sample store of
// a recording instance, the wave's per-environment planes in dynamic LDS, the
// step constants, the sampling tick and the epilogue.
// (The lane mapping is not part of it.  For the plain batch_step_kernel a
// mapping function compiled the instances to different code, measured 2 %
// slower: DESIGN 4.3, and that kernel computes it inline.  The kernels on
// batch_step_body compute theirs inline too and pass the values: there the
// shared body kept registers, LDS and occupancy and measured no slower,
// profiles/batch_unify.)
#pragma once

#include <type_traits>
#include "rb_device.hpp"
#include "rb_internal.hpp"

namespace rb {

// a lane's committed state into slot `slot` of the sample buffer
template <typename T>
__device__ __forceinline__ void sample_store(const BatchParams<T> &p, int32_t slot, int64_t g, const V3<T> &x,
                                             const Q4<T> &q, const V3<T> &v, const V3<T> &w) {
    if (slot < 0 || slot >= p.samp_slots) return;      // (the host's plan keeps a launch inside the buffer)
    const int64_t N = p.E * p.M;
    T *o = p.samp + (int64_t)slot * p.samp_rows * N + g;
    o[0] = x.x; o[N] = x.y; o[2 * N] = x.z;
    o[3 * N] = q.w; o[4 * N] = q.x; o[5 * N] = q.y; o[6 * N] = q.z;
    if (p.samp_rows == 13) {
        o[7 * N] = v.x; o[8 * N] = v.y; o[9 * N] = v.z;
        o[10 * N] = w.x; o[11 * N] = w.y; o[12 * N] = w.z;
    }
}

// The dynamic LDS of the ENVS instances: the planes of the wave's environments
// (one declaration for both real types, hence bytes)
extern __shared__ __align__(16) unsigned char s_env_dyn[];

// The wave's block of per-environment planes, [plane][component][environment
// of the wave] (EnvPlanes, rb_internal.hpp), filled once per launch: from the
// batch's rows, or with the template's planes where no rows are set, so a step
// reads its planes one way.  Lane el < epw fills environment el of the wave.
template <typename T> __device__ __forceinline__ void env_planes_fill(const BatchParams<T> &p, T *blk, int lane, int epw) {
    const int64_t env = (int64_t)blockIdx.x * epw + lane;
    const bool mine = lane < epw;
    const bool live = mine && env < p.E;             // (the rows of environments past the batch are never read)
    for (int a = 0; a < p.n_planes; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            T n = p.pn[a][c], o = p.pp[a][c];
            if (p.env_planes) {
                n = live ? p.env_planes[((int64_t)a * 6 + c) * p.E + env] : T(0);
                o = live ? p.env_planes[((int64_t)a * 6 + 3 + c) * p.E + env] : T(0);
            }
            if (mine) {
                blk[(a * 6 + c) * epw + lane] = n;
                blk[(a * 6 + 3 + c) * epw + lane] = o;
            }
        }
    }
}

// The step constants every law reads (ENVS: the environment's gravity, where set)
template <typename T, bool ENVS>
__device__ __forceinline__ void batch_consts(const BatchParams<T> &p, int64_t ev, StepParams<T> &sp) {
    sp.g[0] = p.g[0]; sp.g[1] = p.g[1]; sp.g[2] = p.g[2];
    sp.dt = p.dt;
    sp.e = p.env_e ? p.env_e[ev] : p.e;
    sp.mu = p.env_mu ? p.env_mu[ev] : p.mu;
    if constexpr (ENVS)
        if (p.env_g) { sp.g[0] = p.env_g[ev]; sp.g[1] = p.env_g[p.E + ev]; sp.g[2] = p.env_g[2 * p.E + ev]; }
}

// REC: steps to the next sample and its slot; a lane ticks after every step and
// on a sampled one stores its committed state (a failed environment's: frozen)
struct SampleTick { int32_t until, slot; };
template <typename T>
__device__ __forceinline__ void sample_tick(const BatchParams<T> &p, SampleTick &t, bool active, int64_t g, const V3<T> &x,
                                            const Q4<T> &q, const V3<T> &v, const V3<T> &w) {
    if (--t.until == 0) {
        if (active) sample_store(p, t.slot, g, x, q, v, w);
        ++t.slot;
        t.until = p.every;
    }
}

// The end of a launch, by an environment's first lane: steps completed, failure code
template <typename T> __device__ __forceinline__ void batch_finish(const BatchParams<T> &p, int b, int64_t env, int32_t done) {
    if (b == 0) {
        if (done > 0) p.steps_done[env] += done;
        if (done < p.k && p.code[env] == 0) p.code[env] = BATCH_EDOM;
    }
}

// a runtime flag as a compile-time constant: f(std::true_type{}) or f(std::false_type{})
template <typename F> static void as_constant(bool flag, F &&f) {
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}

}  // namespace rb
