// rb_world_dev.hip — the device-resident boundary of a world (rb_get_state_dev,
// rb_set_state_dev, rb_set_xfrc_dev): the caller's arrays of structures <-> the
// world's struct-of-arrays rows, both in device memory.  With no PCIe copy
// behind them these transposes are the whole cost of a closed loop's
// iteration, so both sides are moved as contiguous runs through a tile in LDS
// (rb_dev_span.hpp), as the batch's are (rb_batch_dev.hip): a block of SPAN
// threads takes SPAN consecutive bodies; the world's rows are read or written
// one lane per body, contiguously per row.
// What differs from the batch's side: the snapshot's bounding radius comes
// from the constants, box worlds keep a snapshot of the orientations beside
// the positions' (the box narrowphase reads it), the two-ball law's positions
// live in the state rows, and the force rows have pitch S.
#include "rb_world_dev.hpp"
#include "rb_dev_span.hpp"

namespace rb {
namespace {

template <typename T, typename IO, bool VEC>
__global__ __launch_bounds__(SPAN) void wdev_state_in_kernel(WDevState<T> p, const IO *qpos, const IO *qvel) {
    __shared__ IO s_q[SPAN * PITCH], s_v[SPAN * PITCH];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * SPAN;
    const int rows = span_rows(p.N, row0);
    span_load<IO, 7, VEC, false>(qpos + row0 * 7, rows * 7, s_q, nullptr);
    span_load<IO, 6, VEC, false>(qvel + row0 * 6, rows * 6, s_v, nullptr);
    __syncthreads();
    if (t >= rows) return;
    const int64_t b = row0 + t;
    const IO *q = s_q + t * PITCH, *v = s_v + t * PITCH;
    p.snap[b] = Snap<T>{(T)q[0], (T)q[1], (T)q[2], p.bound[b]};
    if (p.quat) {
        T *o = p.quat + 4 * b;
        o[0] = (T)q[3]; o[1] = (T)q[4]; o[2] = (T)q[5]; o[3] = (T)q[6];
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) p.st.row(d)[b] = (T)q[3 + d];
#pragma unroll
    for (int d = 0; d < 6; ++d) p.st.row(4 + d)[b] = (T)v[d];
#pragma unroll
    for (int d = 0; d < 3; ++d) p.st.row(10 + d)[b] = (T)q[d];
}

template <typename T, typename IO, bool VEC>
__global__ __launch_bounds__(SPAN) void wdev_state_out_kernel(WDevState<T> p, IO *qpos, IO *qvel) {
    __shared__ IO s_q[SPAN * PITCH], s_v[SPAN * PITCH];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * SPAN;
    const int rows = span_rows(p.N, row0);
    if (t < rows) {
        const int64_t b = row0 + t;
        if (qpos) {
            IO *q = s_q + t * PITCH;
            if (p.balls) {               // (the snapshot is post-ground: state_out_kernel)
#pragma unroll
                for (int d = 0; d < 3; ++d) q[d] = (IO)p.st.row(10 + d)[b];
            } else {
                const Snap<T> s = p.snap[b];
                q[0] = (IO)s.x; q[1] = (IO)s.y; q[2] = (IO)s.z;
            }
#pragma unroll
            for (int d = 0; d < 4; ++d) q[3 + d] = (IO)p.st.row(d)[b];
        }
        if (qvel) {
            IO *v = s_v + t * PITCH;
#pragma unroll
            for (int d = 0; d < 6; ++d) v[d] = (IO)p.st.row(4 + d)[b];
        }
    }
    __syncthreads();
    if (qpos) span_store<IO, 7, VEC>(qpos + row0 * 7, rows * 7, s_q);
    if (qvel) span_store<IO, 6, VEC>(qvel + row0 * 6, rows * 6, s_v);
}

template <typename T, typename IO, bool VEC>
__global__ __launch_bounds__(SPAN) void wdev_xfrc_in_kernel(const IO *xfrc, T *out, int64_t N, int64_t S) {
    __shared__ IO s_f[SPAN * PITCH];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * SPAN;
    const int rows = span_rows(N, row0);
    span_load<IO, 6, VEC, false>(xfrc + row0 * 6, rows * 6, s_f, nullptr);
    __syncthreads();
    if (t >= rows) return;
#pragma unroll
    for (int d = 0; d < 6; ++d) out[d * S + row0 + t] = (T)s_f[t * PITCH + d];
}

}  // namespace

template <typename T, typename IO>
hipError_t launch_wdev_state_in(const WDevState<T> &p, const IO *qpos, const IO *qvel, hipStream_t s) {
    if (p.N <= 0) return hipSuccess;
    if (!qpos || !qvel) return hipErrorInvalidValue;
    as_flag(aligned16(qpos) && aligned16(qvel), [&](auto VEC) {
        hipLaunchKernelGGL((wdev_state_in_kernel<T, IO, VEC.value>), dim3(spans(p.N)), dim3(SPAN), 0, s, p, qpos, qvel);
    });
    return hipGetLastError();
}

template <typename T, typename IO> hipError_t launch_wdev_state_out(const WDevState<T> &p, IO *qpos, IO *qvel, hipStream_t s) {
    if (p.N <= 0) return hipSuccess;
    if (!qpos && !qvel) return hipErrorInvalidValue;
    as_flag(aligned16(qpos) && aligned16(qvel), [&](auto VEC) {
        hipLaunchKernelGGL((wdev_state_out_kernel<T, IO, VEC.value>), dim3(spans(p.N)), dim3(SPAN), 0, s, p, qpos, qvel);
    });
    return hipGetLastError();
}

template <typename T, typename IO>
hipError_t launch_wdev_xfrc_in(const IO *xfrc, T *rows, int64_t N, int64_t S, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    if (!xfrc || !rows || S < N) return hipErrorInvalidValue;
    as_flag(aligned16(xfrc), [&](auto VEC) {
        hipLaunchKernelGGL((wdev_xfrc_in_kernel<T, IO, VEC.value>), dim3(spans(N)), dim3(SPAN), 0, s, xfrc, rows, N, S);
    });
    return hipGetLastError();
}

#define RB_WDEV_INST(T, IO)                                                                                       \
    template hipError_t launch_wdev_state_in<T, IO>(const WDevState<T> &, const IO *, const IO *, hipStream_t);  \
    template hipError_t launch_wdev_state_out<T, IO>(const WDevState<T> &, IO *, IO *, hipStream_t);             \
    template hipError_t launch_wdev_xfrc_in<T, IO>(const IO *, T *, int64_t, int64_t, hipStream_t);
RB_WDEV_INST(double, double)
RB_WDEV_INST(double, float)
RB_WDEV_INST(float, double)
RB_WDEV_INST(float, float)
#undef RB_WDEV_INST

}  // namespace rb
