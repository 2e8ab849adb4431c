// rb_kat.hip — known-answer kernels (rb_kat_* in include/rbhip.h): one
// primitive of the law per lane on the caller's inputs — the impulse, the
// world inertia and its inverse, the impulse's application and the
// narrowphase of one pair — so tests compare them with the reference's
// values without stepping a world.
#include "rb_device.hpp"
#include "rb_boxes.hpp"
#include "rb_internal.hpp"

namespace rb {

template <typename T>
__global__ void kat_impulse_kernel(int64_t n, const double *in, double *out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const double *a = in + 24 * c;
    const T m = (T)a[0], e = (T)a[1], mu = (T)a[2];
    V3<T> v = {(T)a[3], (T)a[4], (T)a[5]}, w = {(T)a[6], (T)a[7], (T)a[8]};
    const V3<T> r = {(T)a[9], (T)a[10], (T)a[11]}, nn = {(T)a[12], (T)a[13], (T)a[14]};
    M3<T> Iw;
    for (int k = 0; k < 9; ++k) Iw.a[k] = (T)a[15 + k];
    const M3<T> invI = np_inv3(Iw);
    T jn;
    V3<T> jt;
    impulse(impulse_k(m), v, w, r, nn, e, mu, jn, jt);
    apply(v, w, m, invI, r, nn, jn, jt);      // the reference always applies
    double *o = out + 10 * c;
    o[0] = jn; o[1] = jt.x; o[2] = jt.y; o[3] = jt.z;
    o[4] = v.x; o[5] = v.y; o[6] = v.z; o[7] = w.x; o[8] = w.y; o[9] = w.z;
}

template <typename T>
__global__ void kat_inertia_kernel(int64_t n, const double *in, double *out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const double *a = in + 7 * c;
    const M3<T> Iw = inertia_world(V3<T>{(T)a[0], (T)a[1], (T)a[2]}, Q4<T>{(T)a[3], (T)a[4], (T)a[5], (T)a[6]});
    const M3<T> Ii = np_inv3(Iw);
    for (int k = 0; k < 9; ++k) { out[18 * c + k] = Iw.a[k]; out[18 * c + 9 + k] = Ii.a[k]; }
}

template <typename T>
__global__ void kat_apply_kernel(int64_t n, const double *in, double *out) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const double *a = in + 26 * c;
    const T m = (T)a[0];
    V3<T> v = {(T)a[1], (T)a[2], (T)a[3]}, w = {(T)a[4], (T)a[5], (T)a[6]};
    const V3<T> r = {(T)a[7], (T)a[8], (T)a[9]}, nn = {(T)a[10], (T)a[11], (T)a[12]};
    const T jn = (T)a[13];
    const V3<T> jt = {(T)a[14], (T)a[15], (T)a[16]};
    M3<T> Iw;
    for (int k = 0; k < 9; ++k) Iw.a[k] = (T)a[17 + k];
    apply(v, w, m, np_inv3(Iw), r, nn, jn, jt);
    double *o = out + 6 * c;
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = w.x; o[4] = w.y; o[5] = w.z;
}

// in[22] = kind1, kind2, c1[3], q1[4], s1[3], c2[3], q2[4], s2[3] (body 1 =
// lower id) -> out[33] = count, then per contact dist, pos[3], frame[3], kind
template <typename T>
__global__ __launch_bounds__(64) void kat_narrow_kernel(int64_t n, const double *in, double *out) {
    __shared__ T s_poly[48 * 64];
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const double *a = in + 22 * c;
    double *o = out + 33 * c;
    for (int k = 0; k < 33; ++k) o[k] = 0;
    const int k1 = (int)a[0], k2 = (int)a[1];
    const V3<T> c1 = {(T)a[2], (T)a[3], (T)a[4]}, c2 = {(T)a[12], (T)a[13], (T)a[14]};
    const Q4<T> q1 = {(T)a[5], (T)a[6], (T)a[7], (T)a[8]}, q2 = {(T)a[15], (T)a[16], (T)a[17], (T)a[18]};
    const V3<T> s1 = {(T)a[9], (T)a[10], (T)a[11]}, s2 = {(T)a[19], (T)a[20], (T)a[21]};
    int m = 0;
    auto emit = [&](const Contact<T> &con, int ck) {
        double *r = o + 1 + 8 * m;
        r[0] = (double)con.dist;
        r[1] = (double)con.pos.x; r[2] = (double)con.pos.y; r[3] = (double)con.pos.z;
        r[4] = (double)con.frame.x; r[5] = (double)con.frame.y; r[6] = (double)con.frame.z;
        r[7] = ck;
        ++m;
    };
    Contact<T> con;
    if (k1 == 0 && k2 == 0) {
        if (sphere_sphere(c1, s1.x, c2, s2.x, con)) emit(con, 16);
    } else if (k1 == 0) {
        if (sphere_box(c1, s1.x, c2, mj_body_mat(q2), s2, con)) emit(con, CK_SPHERE_BOX);
    } else if (k2 == 0) {
        if (sphere_box(c2, s2.x, c1, mj_body_mat(q1), s1, con)) emit(con, CK_SPHERE_BOX);
    } else {
        box_box(c1, mj_body_mat(q1), s1, c2, mj_body_mat(q2), s2, s_poly + threadIdx.x, 64, emit);
    }
    o[0] = m;
}

template <typename T> hipError_t launch_kat_impulse(int64_t n, const double *in, double *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((kat_impulse_kernel<T>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, n, in, out);
    return hipGetLastError();
}

template <typename T> hipError_t launch_kat_inertia(int64_t n, const double *in, double *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((kat_inertia_kernel<T>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, n, in, out);
    return hipGetLastError();
}

template <typename T> hipError_t launch_kat_apply(int64_t n, const double *in, double *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((kat_apply_kernel<T>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, n, in, out);
    return hipGetLastError();
}

template <typename T> hipError_t launch_kat_narrow(int64_t n, const double *in, double *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((kat_narrow_kernel<T>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, n, in, out);
    return hipGetLastError();
}

#define RB_KAT_INST(T)                                                                                         \
    template hipError_t launch_kat_impulse<T>(int64_t, const double *, double *, hipStream_t);                \
    template hipError_t launch_kat_inertia<T>(int64_t, const double *, double *, hipStream_t);                \
    template hipError_t launch_kat_apply<T>(int64_t, const double *, double *, hipStream_t);                  \
    template hipError_t launch_kat_narrow<T>(int64_t, const double *, double *, hipStream_t);
RB_KAT_INST(double)
RB_KAT_INST(float)
#undef RB_KAT_INST

}  // namespace rb
