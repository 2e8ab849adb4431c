// rb_step_wide.hip — the wide forms of the step kernel (one lane per body at
// one wave per SIMD, with and without a helper wave; the body: rb_step.hpp)
// and their launcher.  A unit of their own because they are built with the
// memory-clause scheduling flags (Makefile KFLAGS); rb_internal.hpp declares
// launch_step_wide extern, so no other unit can compile a copy.
// Built once per real type: RB_INST = 1 fp64, 2 fp32.
#include "rb_device.hpp"

// diagnostic build only (rb_step.hpp STAMP): the stamp buffer, in the fp64
// object (its host-side name must be unique in the library)
#ifndef RB_STAMPS
#define RB_STAMPS 0
#endif
#if RB_INST != 1
#undef RB_STAMPS
#define RB_STAMPS 0
#endif
#if RB_STAMPS
__device__ unsigned long long rb_stamp_buf[1 << 16][16];
__device__ unsigned long long rb_stamp_buf_help[1 << 16][16];   // the helper wave's (shared search)
#endif
#include "rb_step.hpp"

#if RB_STAMPS
extern "C" int rb_diag_stamps(unsigned long long *out, int nblocks) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(rb_stamp_buf), sizeof(unsigned long long) * 16 * nblocks);
}
extern "C" int rb_diag_stamps_help(unsigned long long *out, int nblocks) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(rb_stamp_buf_help), sizeof(unsigned long long) * 16 * nblocks);
}
#endif

namespace rb {

// one wave per SIMD (up to 64 x 1024 owned bodies): every register is free
template <typename T, int MAXP, bool HALO>
__global__ __launch_bounds__(STEP_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1)))
void step_kernel_wide(const Snap<T> *snap_cur, T *st_base, int64_t st_S, const T *cs_base, int64_t cs_Npad,
                      const int32_t *cs_kind, int32_t n_local, int32_t lo, StepParams<T> p) {
    step_body<T, MAXP, 1, true, false, false, HALO>(
        p, Lead<T>{snap_cur, BodyState<T>{st_base, st_S}, BodyConsts<T>{cs_base, cs_Npad, cs_kind}, n_local, lo});
}

// the wide form with a helper wave per workgroup (help_body): two waves per
// SIMD, each within 256 registers
// SHARE: the helper lanes also search half of each body's 2x2x2
// neighbourhood (rb_grid.hpp search_half_wide) and finish the body
template <typename T, int MAXP, bool HALO, bool SHARE>
__global__ __launch_bounds__(2 * STEP_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2)))
void step_kernel_wide_help(const Snap<T> *snap_cur, T *st_base, int64_t st_S, const T *cs_base, int64_t cs_Npad,
                           const int32_t *cs_kind, int32_t n_local, int32_t lo, StepParams<T> p) {
    step_body<T, MAXP, 1, true, false, true, HALO, false, SHARE>(
        p, Lead<T>{snap_cur, BodyState<T>{st_base, st_S}, BodyConsts<T>{cs_base, cs_Npad, cs_kind}, n_local, lo});
}

// The instances of worlds with append epochs (never halo-exchanging): the
// lead that carries the lead block's address (rb_step.hpp LEAD_EP_*), so the
// epoch control word arrives with the parameter block, not after it
template <typename T, int MAXP>
__global__ __launch_bounds__(STEP_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1)))
void step_kernel_wide_ep(LEAD_EP_PARAMS(T), StepParams<T> p) {
    step_body<T, MAXP, 1, true, false, false, false, true>(p, LEAD_EP_OF(T));
}
template <typename T, int MAXP, bool SHARE>
__global__ __launch_bounds__(2 * STEP_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2)))
void step_kernel_wide_help_ep(LEAD_EP_PARAMS(T), StepParams<T> p) {
    step_body<T, MAXP, 1, true, false, true, false, true, SHARE>(p, LEAD_EP_OF(T));
}

template <typename T> hipError_t launch_step_wide(const StepParams<T> &p, int maxp, bool help, bool share, hipStream_t s) {
    int64_t blocks = (p.n_local + STEP_BLOCK - 1) / STEP_BLOCK;
    if (blocks < 1) blocks = 1;
    const bool halo = p.halo.mail != nullptr;
    // worlds with append epochs (never halo-exchanging: rb_api_step.hip
    // epoch_eligible) launch the instantiation that carries the epoch code
    const bool ep = p.ep.ctrl != nullptr && !halo;
#define RB_WIDE_LAUNCH(K, M, H, TH)                                                                               \
    hipLaunchKernelGGL((K<T, M, H>), dim3((unsigned)blocks), dim3(TH), 0, s, LEAD_ARGS(p), p)
#define RB_WIDE_HELP_EP_LAUNCH(M, TH)                                                                             \
    do {                                                                                                          \
        if (share) hipLaunchKernelGGL((step_kernel_wide_help_ep<T, M, true>), dim3((unsigned)blocks), dim3(TH), 0, s, LEAD_EP_ARGS(p), p); \
        else hipLaunchKernelGGL((step_kernel_wide_help_ep<T, M, false>), dim3((unsigned)blocks), dim3(TH), 0, s, LEAD_EP_ARGS(p), p); \
    } while (0)
#define RB_WIDE_HELP_LAUNCH(M, H, TH)                                                                             \
    do {                                                                                                          \
        if (share) hipLaunchKernelGGL((step_kernel_wide_help<T, M, H, true>), dim3((unsigned)blocks), dim3(TH), 0, s, LEAD_ARGS(p), p); \
        else hipLaunchKernelGGL((step_kernel_wide_help<T, M, H, false>), dim3((unsigned)blocks), dim3(TH), 0, s, LEAD_ARGS(p), p); \
    } while (0)
#define RB_WIDE_PICK(K, M, TH)                                                                                    \
    do {                                                                                                          \
        if (halo) RB_WIDE_LAUNCH(K, M, true, TH);                                                                 \
        else if (ep) hipLaunchKernelGGL((K##_ep<T, M>), dim3((unsigned)blocks), dim3(TH), 0, s, LEAD_EP_ARGS(p), p); \
        else RB_WIDE_LAUNCH(K, M, false, TH);                                                                     \
    } while (0)
    if (help) {
#define RB_WIDE_HELP_PICK(M)                                                                                      \
    do {                                                                                                          \
        if (halo) RB_WIDE_HELP_LAUNCH(M, true, 2 * STEP_BLOCK);                                                   \
        else if (ep) RB_WIDE_HELP_EP_LAUNCH(M, 2 * STEP_BLOCK);                                                   \
        else RB_WIDE_HELP_LAUNCH(M, false, 2 * STEP_BLOCK);                                                       \
    } while (0)
        if (maxp <= 16) RB_WIDE_HELP_PICK(16);
        else RB_WIDE_HELP_PICK(32);
#undef RB_WIDE_HELP_PICK
#undef RB_WIDE_HELP_LAUNCH
#undef RB_WIDE_HELP_EP_LAUNCH
        return hipGetLastError();
    }
    if (maxp <= 16) RB_WIDE_PICK(step_kernel_wide, 16, STEP_BLOCK);
    else RB_WIDE_PICK(step_kernel_wide, 32, STEP_BLOCK);
#undef RB_WIDE_PICK
#undef RB_WIDE_LAUNCH
    return hipGetLastError();
}

#if RB_INST == 1
using Real = double;
#elif RB_INST == 2
using Real = float;
#else
#error "RB_INST: 1 (fp64) or 2 (fp32)"
#endif
template hipError_t launch_step_wide<Real>(const StepParams<Real> &, int, bool, bool, hipStream_t);

}  // namespace rb
