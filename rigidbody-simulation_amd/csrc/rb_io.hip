// rb_io.hip — kernels around the step, none of them on the hot path: the
// table insert of a body range (world set-up, shard exchange) and the state
// across the boundary (rb_set_state / rb_get_state), with their launchers.
#include <algorithm>

#include "rb_device.hpp"
#include "rb_grid.hpp"
#include "rb_internal.hpp"

namespace rb {

template <typename T>
__global__ __launch_bounds__(256) void insert_kernel(InsertParams<T> p) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= p.count) return;
    const int64_t id = p.first + k;
    if (id >= p.skip_lo && id < p.skip_hi) return;
    insert_id(p.grid, p.tab, p.err, p.snap[id], (uint32_t)id | (p.kind[id] != 0 ? BOX_FLAG : 0u), *p.tab.gen);
}

// ---- the state across the boundary (rb_set_state / rb_get_state) ----------
// One lane per body: AoS rows of the caller (qpos[7k], qvel[6k], D1-fixed
// multi_sphere_bounce.py layout) <-> SoA state rows and snapshot.  The host
// moves the rows with one DMA each way (pinned staging, rb_api_state.hip).
template <typename T>
__global__ __launch_bounds__(256) void state_in_kernel(StateIO<T> p) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.N) return;
    const double *q = p.qpos + 7 * b;
    p.snap[b] = Snap<T>{(T)q[0], (T)q[1], (T)q[2], p.bound[b]};
    if (p.quat) {
        T *o = p.quat + 4 * b;
        o[0] = (T)q[3]; o[1] = (T)q[4]; o[2] = (T)q[5]; o[3] = (T)q[6];
    }
    const int64_t l = b - p.lo;
    if (l < 0 || l >= p.n_local) return;
    const double *v = p.qvel + 6 * b;
#pragma unroll
    for (int d = 0; d < 4; ++d) p.st.row(d)[l] = (T)q[3 + d];
#pragma unroll
    for (int d = 0; d < 6; ++d) p.st.row(4 + d)[l] = (T)v[d];
#pragma unroll
    for (int d = 0; d < 3; ++d) p.st.row(10 + d)[l] = (T)q[d];
}

template <typename T>
__global__ __launch_bounds__(256) void state_out_kernel(StateIO<T> p, int want_q, int want_v) {
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= p.n_local) return;
    const int64_t b = p.lo + l;
    if (want_q) {
        double *q = p.qpos + 7 * b;
        if (p.balls) {
#pragma unroll
            for (int d = 0; d < 3; ++d) q[d] = (double)p.st.row(10 + d)[l];
        } else {
            const Snap<T> s = p.snap[b];
            q[0] = (double)s.x; q[1] = (double)s.y; q[2] = (double)s.z;
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) q[3 + d] = (double)p.st.row(d)[l];
    }
    if (want_v) {
        double *v = p.qvel + 6 * b;
#pragma unroll
        for (int d = 0; d < 6; ++d) v[d] = (double)p.st.row(4 + d)[l];
    }
}

// The same rows written straight into mapped pinned host memory (p.qpos /
// p.qvel host-mapped): one lane per output double, so every wave's store is
// one contiguous 512 B run across PCIe (a lane per body would scatter 56 B
// strides); the SoA rows are gathered from HBM instead.
template <typename T>
__global__ __launch_bounds__(256) void state_out_flat_kernel(StateIO<T> p, int want_q, int want_v) {
    const int64_t nq = want_q ? 7 * (int64_t)p.n_local : 0, nv = want_v ? 6 * (int64_t)p.n_local : 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nq + nv; e += (int64_t)gridDim.x * blockDim.x) {
        if (e < nq) {
            const int64_t l = e / 7;
            const int d = (int)(e - 7 * l);
            T x;
            if (d >= 3) x = p.st.row(d - 3)[l];
            else if (p.balls) x = p.st.row(10 + d)[l];
            else x = reinterpret_cast<const T *>(p.snap + p.lo + l)[d];
            p.qpos[7 * p.lo + e] = (double)x;
        } else {
            const int64_t f = e - nq, l = f / 6;
            const int d = (int)(f - 6 * l);
            p.qvel[6 * p.lo + f] = (double)p.st.row(4 + d)[l];
        }
    }
}

template <typename T> hipError_t launch_state_in(const StateIO<T> &p, hipStream_t s) {
    if (p.N <= 0) return hipSuccess;
    hipLaunchKernelGGL((state_in_kernel<T>), dim3((unsigned)((p.N + 255) / 256)), dim3(256), 0, s, p);
    return hipGetLastError();
}
template <typename T> hipError_t launch_state_out(const StateIO<T> &p, bool want_q, bool want_v, hipStream_t s) {
    if (p.n_local <= 0) return hipSuccess;
    hipLaunchKernelGGL((state_out_kernel<T>), dim3((unsigned)((p.n_local + 255) / 256)), dim3(256), 0, s, p,
                       want_q ? 1 : 0, want_v ? 1 : 0);
    return hipGetLastError();
}
template <typename T> hipError_t launch_state_out_flat(const StateIO<T> &p, bool want_q, bool want_v, hipStream_t s) {
    if (p.n_local <= 0) return hipSuccess;
    const int64_t n = 13 * (int64_t)p.n_local;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL((state_out_flat_kernel<T>), dim3(blocks), dim3(256), 0, s, p, want_q ? 1 : 0, want_v ? 1 : 0);
    return hipGetLastError();
}

template <typename T> hipError_t launch_insert(const InsertParams<T> &p, hipStream_t s) {
    if (p.count <= 0) return hipSuccess;
    const int64_t blocks = (p.count + 255) / 256;
    hipLaunchKernelGGL((insert_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

#define RB_IO_INST(T)                                                                                          \
    template hipError_t launch_insert<T>(const InsertParams<T> &, hipStream_t);                               \
    template hipError_t launch_state_in<T>(const StateIO<T> &, hipStream_t);                                  \
    template hipError_t launch_state_out<T>(const StateIO<T> &, bool, bool, hipStream_t);                     \
    template hipError_t launch_state_out_flat<T>(const StateIO<T> &, bool, bool, hipStream_t);
RB_IO_INST(double)
RB_IO_INST(float)
#undef RB_IO_INST

}  // namespace rb
