// rb_api_kat.hip — the known-answer entries (rb_kat_*): device functions run
// on caller-supplied rows, for the tests against the reference goldens.
#include "rb_host.hpp"

using namespace rb::host;

static int kat_common(int32_t device, int32_t dtype, int64_t n, const double *in, double *out, int nin, int nout,
                      int which) {
    if (n < 0 || (n && (!in || !out))) return fail(RB_EINVAL, "bad KAT arguments");
    if (dtype != RB_F64 && dtype != RB_F32) return fail(RB_EINVAL, "bad dtype");
    if (n == 0) return RB_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(RB_ENODEV, "no HIP device available");
    HIPCHK(hipSetDevice(device));
    DevBuf<double> din, dout;
    WCHK(din.alloc(sizeof(double) * nin * n));
    WCHK(dout.alloc(sizeof(double) * nout * n));
    hipError_t e = hipMemcpy(din, in, sizeof(double) * nin * n, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = by_real(dtype, [&](auto t) {
            using T = decltype(t);
            return which == 1   ? launch_kat_inertia<T>(n, din, dout, nullptr)
                   : which == 2 ? launch_kat_apply<T>(n, din, dout, nullptr)
                   : which == 3 ? launch_kat_pair_impulse<T>(n, din, dout, nullptr)
                   : which == 4 ? launch_kat_narrow<T>(n, din, dout, nullptr)
                                : launch_kat_impulse<T>(n, din, dout, nullptr);
        });
    if (e == hipSuccess) e = hipMemcpy(out, dout, sizeof(double) * nout * n, hipMemcpyDeviceToHost);
    HIPCHK(e);
    return RB_OK;
}

extern "C" {

int rb_kat_impulse(int32_t device, int32_t dtype, int64_t n, const double *in, double *out) {
    ApiScope api_scope_(device);
    return kat_common(device, dtype, n, in, out, 24, 10, 0);
}

int rb_kat_inertia(int32_t device, int32_t dtype, int64_t n, const double *in, double *out) {
    ApiScope api_scope_(device);
    return kat_common(device, dtype, n, in, out, 7, 18, 1);
}

int rb_kat_apply(int32_t device, int32_t dtype, int64_t n, const double *in, double *out) {
    ApiScope api_scope_(device);
    return kat_common(device, dtype, n, in, out, 26, 6, 2);
}

int rb_kat_pair_impulse(int32_t device, int32_t dtype, int64_t n, const double *in, double *out) {
    ApiScope api_scope_(device);
    return kat_common(device, dtype, n, in, out, 27, 3, 3);
}

int rb_kat_narrow(int32_t device, int32_t dtype, int64_t n, const double *in, double *out) {
    ApiScope api_scope_(device);
    return kat_common(device, dtype, n, in, out, 22, 33, 4);
}

}  // extern "C"
