// rb_batch_dev.hip — the device-resident boundary of a batch (rb_batch_*_dev):
// the caller's arrays of structures <-> the batch's struct-of-arrays rows, both
// in device memory.  With no PCIe copy behind them these transposes are the
// whole cost of a closed loop's iteration, so both sides are moved as
// contiguous runs through a tile in LDS (rb_dev_span.hpp): a block of SPAN
// threads takes SPAN consecutive rows (body slots); the rows of the batch are
// read or written one lane per slot, contiguously per row.
#include <math.h>

#include <algorithm>

#include "rb_batch_dev.hpp"
#include "rb_dev_span.hpp"

namespace rb {
namespace {

template <typename T, typename IO, bool VEC, bool MASKED>
__global__ __launch_bounds__(SPAN) void dev_state_in_kernel(DevState<T> p, const uint8_t *mask, const IO *qpos,
                                                            const IO *qvel) {
    __shared__ IO s_q[SPAN * PITCH], s_v[SPAN * PITCH];
    __shared__ uint8_t s_env[SPAN], s_row[SPAN];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * SPAN;
    const int rows = span_rows(p.N, row0);
    // the environments with a row in this span (at most SPAN): lane t takes
    // one, reads its mask byte once and, in the block that holds the
    // environment's first row, resets it
    const int64_t env0 = row0 / p.M;
    const int n_env = (int)((row0 + rows - 1) / p.M - env0) + 1;
    if (t < n_env) {
        const int64_t e = env0 + t;
        const bool on = !MASKED || mask[e] != 0;
        if (MASKED) s_env[t] = on;
        if (on && e * p.M >= row0) {
            p.code[e] = 0;
            p.steps_done[e] = 0;
        }
    }
    if (MASKED) {
        __syncthreads();
        if (t < rows) s_row[t] = s_env[(row0 + t) / p.M - env0];
        __syncthreads();
    }
    span_load<IO, 7, VEC, MASKED>(qpos + row0 * 7, rows * 7, s_q, s_row);
    span_load<IO, 6, VEC, MASKED>(qvel + row0 * 6, rows * 6, s_v, s_row);
    __syncthreads();
    if (t >= rows || (MASKED && !s_row[t])) return;
    const int64_t g = row0 + t;
    const IO *q = s_q + t * PITCH, *v = s_v + t * PITCH;
    p.snap[g] = Snap<T>{(T)q[0], (T)q[1], (T)q[2], p.bound[g]};
#pragma unroll
    for (int d = 0; d < 4; ++d) p.st.row(d)[g] = (T)q[3 + d];
#pragma unroll
    for (int d = 0; d < 6; ++d) p.st.row(4 + d)[g] = (T)v[d];
#pragma unroll
    for (int d = 0; d < 3; ++d) p.st.row(10 + d)[g] = (T)q[d];
}

template <typename T, typename IO, bool VEC>
__global__ __launch_bounds__(SPAN) void dev_state_out_kernel(DevState<T> p, IO *qpos, IO *qvel) {
    __shared__ IO s_q[SPAN * PITCH], s_v[SPAN * PITCH];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * SPAN;
    const int rows = span_rows(p.N, row0);
    if (t < rows) {
        const int64_t g = row0 + t;
        if (qpos) {
            IO *q = s_q + t * PITCH;
            const Snap<T> s = p.snap[g];
            q[0] = (IO)s.x; q[1] = (IO)s.y; q[2] = (IO)s.z;
#pragma unroll
            for (int d = 0; d < 4; ++d) q[3 + d] = (IO)p.st.row(d)[g];
        }
        if (qvel) {
            IO *v = s_v + t * PITCH;
#pragma unroll
            for (int d = 0; d < 6; ++d) v[d] = (IO)p.st.row(4 + d)[g];
        }
    }
    __syncthreads();
    if (qpos) span_store<IO, 7, VEC>(qpos + row0 * 7, rows * 7, s_q);
    if (qvel) span_store<IO, 6, VEC>(qvel + row0 * 6, rows * 6, s_v);
}

template <typename IO, bool VEC>
__global__ __launch_bounds__(SPAN) void dev_xfrc_check_kernel(const IO *xfrc, int64_t N, uint32_t *refused) {
    using R = Run<IO, VEC>;
    const int64_t row0 = (int64_t)blockIdx.x * SPAN;
    const int n = span_rows(N, row0) * 6, nv = n / R::V;
    const IO *src = xfrc + row0 * 6;
    uint32_t bad = DEV_NO_SLOT;
    for (int i = threadIdx.x; i < nv; i += SPAN) {
        const int f = i * R::V;
        const typename R::Vec x = *reinterpret_cast<const typename R::Vec *>(src + f);
#pragma unroll
        for (int j = 0; j < R::V; ++j)
            if (!isfinite(x.v[j])) bad = min(bad, (uint32_t)(row0 + (f + j) / 6));
    }
    for (int f = nv * R::V + threadIdx.x; f < n; f += SPAN)
        if (!isfinite(src[f])) bad = min(bad, (uint32_t)(row0 + f / 6));
    if (bad != DEV_NO_SLOT) atomicMin(refused, bad);
}

template <typename T, typename IO, bool VEC>
__global__ __launch_bounds__(SPAN) void dev_xfrc_in_kernel(const IO *xfrc, T *out, int64_t N, const uint32_t *refused) {
    __shared__ IO s_f[SPAN * PITCH];
    if (*refused != DEV_NO_SLOT) return;     // (one word, written before this launch: the same for every lane)
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * SPAN;
    const int rows = span_rows(N, row0);
    span_load<IO, 6, VEC, false>(xfrc + row0 * 6, rows * 6, s_f, nullptr);
    __syncthreads();
    if (t >= rows) return;
#pragma unroll
    for (int d = 0; d < 6; ++d) out[d * N + row0 + t] = (T)s_f[t * PITCH + d];
}

// a block: one span of one sample (bps spans per sample)
template <typename T, typename IO, bool VEC>
__global__ __launch_bounds__(SPAN) void dev_samples_out_kernel(const T *samp, int32_t rows_per, int64_t N, int32_t bps,
                                                              IO *qpos, IO *qvel) {
    __shared__ IO s_q[SPAN * PITCH], s_v[SPAN * PITCH];
    const int t = threadIdx.x;
    const int64_t k = blockIdx.x / bps;
    const int64_t row0 = (int64_t)(blockIdx.x - k * bps) * SPAN;
    const int rows = span_rows(N, row0);
    const bool vel = rows_per == 13;
    if (t < rows) {
        const T *in = samp + k * rows_per * N + row0 + t;
#pragma unroll
        for (int d = 0; d < 7; ++d) s_q[t * PITCH + d] = (IO)in[d * N];
        if (vel) {
#pragma unroll
            for (int d = 0; d < 6; ++d) s_v[t * PITCH + d] = (IO)in[(7 + d) * N];
        }
    }
    __syncthreads();
    span_store<IO, 7, VEC>(qpos + (k * N + row0) * 7, rows * 7, s_q);
    if (vel) span_store<IO, 6, VEC>(qvel + (k * N + row0) * 6, rows * 6, s_v);
}

}  // namespace

template <typename T, typename IO>
hipError_t launch_dev_state_in(const DevState<T> &p, const uint8_t *mask, const IO *qpos, const IO *qvel, hipStream_t s) {
    if (p.N <= 0) return hipSuccess;
    if (!qpos || !qvel || p.M < 1) return hipErrorInvalidValue;
    as_flag(aligned16(qpos) && aligned16(qvel), [&](auto VEC) {
        as_flag(mask != nullptr, [&](auto MASKED) {
            hipLaunchKernelGGL((dev_state_in_kernel<T, IO, VEC.value, MASKED.value>), dim3(spans(p.N)), dim3(SPAN), 0, s, p,
                               mask, qpos, qvel);
        });
    });
    return hipGetLastError();
}

template <typename T, typename IO> hipError_t launch_dev_state_out(const DevState<T> &p, IO *qpos, IO *qvel, hipStream_t s) {
    if (p.N <= 0) return hipSuccess;
    if (!qpos && !qvel) return hipErrorInvalidValue;
    as_flag(aligned16(qpos) && aligned16(qvel), [&](auto VEC) {
        hipLaunchKernelGGL((dev_state_out_kernel<T, IO, VEC.value>), dim3(spans(p.N)), dim3(SPAN), 0, s, p, qpos, qvel);
    });
    return hipGetLastError();
}

template <typename IO> hipError_t launch_dev_xfrc_check(const IO *xfrc, int64_t N, uint32_t *refused, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    if (!xfrc || !refused) return hipErrorInvalidValue;
    as_flag(aligned16(xfrc), [&](auto VEC) {
        hipLaunchKernelGGL((dev_xfrc_check_kernel<IO, VEC.value>), dim3(spans(N)), dim3(SPAN), 0, s, xfrc, N, refused);
    });
    return hipGetLastError();
}

template <typename T, typename IO>
hipError_t launch_dev_xfrc_in(const IO *xfrc, T *rows, int64_t N, const uint32_t *refused, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    if (!xfrc || !rows || !refused) return hipErrorInvalidValue;
    as_flag(aligned16(xfrc), [&](auto VEC) {
        hipLaunchKernelGGL((dev_xfrc_in_kernel<T, IO, VEC.value>), dim3(spans(N)), dim3(SPAN), 0, s, xfrc, rows, N, refused);
    });
    return hipGetLastError();
}

template <typename T, typename IO>
hipError_t launch_dev_samples_out(const T *samp, int32_t n, int32_t rows, int64_t N, IO *qpos, IO *qvel, hipStream_t s) {
    if (n <= 0 || N <= 0) return hipSuccess;
    if (!samp || !qpos || (rows != 7 && rows != 13) || (rows == 13 && !qvel)) return hipErrorInvalidValue;
    const int64_t blocks = (int64_t)spans(N) * n;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    // every sample's run starts where the one before ends: aligned when the base and a sample's size are
    const bool vec = aligned16(qpos) && aligned16(qvel) && (n == 1 || (N * 7 * sizeof(IO) % 16 == 0 && N * 6 * sizeof(IO) % 16 == 0));
    as_flag(vec, [&](auto VEC) {
        hipLaunchKernelGGL((dev_samples_out_kernel<T, IO, VEC.value>), dim3((unsigned)blocks), dim3(SPAN), 0, s, samp, rows, N,
                           (int32_t)spans(N), qpos, qvel);
    });
    return hipGetLastError();
}

#define RB_DEV_INST(T, IO)                                                                                               \
    template hipError_t launch_dev_state_in<T, IO>(const DevState<T> &, const uint8_t *, const IO *, const IO *, hipStream_t); \
    template hipError_t launch_dev_state_out<T, IO>(const DevState<T> &, IO *, IO *, hipStream_t);                      \
    template hipError_t launch_dev_xfrc_in<T, IO>(const IO *, T *, int64_t, const uint32_t *, hipStream_t);             \
    template hipError_t launch_dev_samples_out<T, IO>(const T *, int32_t, int32_t, int64_t, IO *, IO *, hipStream_t);
RB_DEV_INST(double, double)
RB_DEV_INST(double, float)
RB_DEV_INST(float, double)
RB_DEV_INST(float, float)
#undef RB_DEV_INST
template hipError_t launch_dev_xfrc_check<double>(const double *, int64_t, uint32_t *, hipStream_t);
template hipError_t launch_dev_xfrc_check<float>(const float *, int64_t, uint32_t *, hipStream_t);

}  // namespace rb
