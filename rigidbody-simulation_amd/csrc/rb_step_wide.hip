// rb_step_wide.hip — the wide forms of the step kernel (one lane per body at
// one wave per SIMD, with and without a helper wave; the body: rb_step.hpp)
// and their launcher.  Each kernel names its form (rb_step.hpp FormDefaults:
// Wide, WideHelp, WideEp, WideHelpEp) and, beside it, whether the halo push
// is compiled in.  A unit of their own because they are built with the
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
void step_kernel_wide(LEAD_PARAMS(T), StepParams<T> p) {
    step_body<T, Wide<MAXP>, HALO>(p, LEAD_OF(T));
}

// the wide form with a helper wave per workgroup (help_body): two waves per
// SIMD, each within 256 registers
// SHARE: the helper lanes also search half of each body's 2x2x2
// neighbourhood (rb_grid.hpp search_half_wide) and finish the body
template <typename T, int MAXP, bool HALO, bool SHARE>
__global__ __launch_bounds__(2 * STEP_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2)))
void step_kernel_wide_help(LEAD_PARAMS(T), StepParams<T> p) {
    step_body<T, WideHelp<MAXP, SHARE>, HALO>(p, LEAD_OF(T));
}

// The instances of worlds with append epochs (never halo-exchanging): the
// lead that carries the lead block's address (rb_step.hpp LEAD_EP_*), so the
// epoch control word arrives with the parameter block, not after it
template <typename T, int MAXP>
__global__ __launch_bounds__(STEP_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1)))
void step_kernel_wide_ep(LEAD_EP_PARAMS(T), StepParams<T> p) {
    step_body<T, WideEp<MAXP>, false>(p, LEAD_EP_OF(T));
}
template <typename T, int MAXP, bool SHARE>
__global__ __launch_bounds__(2 * STEP_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2)))
void step_kernel_wide_help_ep(LEAD_EP_PARAMS(T), StepParams<T> p) {
    step_body<T, WideHelpEp<MAXP, SHARE>, false>(p, LEAD_EP_OF(T));
}

template <typename T> hipError_t launch_step_wide(const StepParams<T> &p, int maxp, bool help, bool share, hipStream_t s) {
    int64_t blocks = (p.n_local + STEP_BLOCK - 1) / STEP_BLOCK;
    if (blocks < 1) blocks = 1;
    const bool halo = p.halo.mail != nullptr;
    // worlds with append epochs (never halo-exchanging: rb_api_step.hip
    // epoch_eligible) launch the instantiation that carries the epoch code
    const bool ep = p.ep.ctrl != nullptr && !halo;
    const dim3 grid((unsigned)blocks), one(STEP_BLOCK), two(2 * STEP_BLOCK);
    const bool m16 = maxp <= 16;
    // (the choices in this order, and the _ep kernels between the two halo
    // choices: the order the instances are compiled in)
    if (help)
        pick([&](auto m, auto h, auto e, auto sh) {
            constexpr int M = maxp_c(m.value);
            if constexpr (e.value && !h.value) hipLaunchKernelGGL((step_kernel_wide_help_ep<T, M, sh.value>), grid, two, 0, s, LEAD_EP_ARGS(p), p);
            else hipLaunchKernelGGL((step_kernel_wide_help<T, M, h.value, sh.value>), grid, two, 0, s, LEAD_ARGS(p), p);
        }, m16, halo, ep, share);
    else
        pick([&](auto m, auto h, auto e) {
            constexpr int M = maxp_c(m.value);
            if constexpr (e.value && !h.value) hipLaunchKernelGGL((step_kernel_wide_ep<T, M>), grid, one, 0, s, LEAD_EP_ARGS(p), p);
            else hipLaunchKernelGGL((step_kernel_wide<T, M, h.value>), grid, one, 0, s, LEAD_ARGS(p), p);
        }, m16, halo, ep);
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
