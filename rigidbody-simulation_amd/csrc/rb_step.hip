// rb_step.hip — the step kernels built with the default scheduling (the body
// they share with the wide forms: rb_step.hpp): the cooperative form, with
// and without a helper wave, the one-lane form, the box kernel, the split
// form's search and update kernels, and launch_step, which picks among them
// (the wide forms through rb_step_wide.hip's launch_step_wide).  Each kernel
// names its form (rb_step.hpp FormDefaults: Coop, CoopHelp, One, BoxBody,
// SplitUpdate); the launcher turns maxp into a constant with pick().
// Built once per real type: RB_INST = 1 fp64, 2 fp32.

// the phase stamps are the wide unit's (rb_step_wide.hip)
#undef RB_STAMPS
#define RB_STAMPS 0
#include "rb_step.hpp"

namespace rb {

// The two forms as separate kernels: the one-lane (large-scene) form may be
// compiled for more waves per SIMD — its dependent random loads want
// occupancy more than registers — without touching the cooperative form.
#ifndef RB_MIN_WAVES_G1
#define RB_MIN_WAVES_G1 1
#endif
// the cooperative form fits 3 waves per SIMD without spilling (measured:
// +9-12% at 32k-65k bodies, unchanged at 4k; 4 waves spill and lose)
#ifndef RB_MIN_WAVES_COOP
#define RB_MIN_WAVES_COOP 3
#endif
template <typename T, int MAXP>
__global__ __launch_bounds__(STEP_BLOCK)
__attribute__((amdgpu_waves_per_eu(MAXP <= 16 ? RB_MIN_WAVES_COOP : 2)))   // 32 partners: 2 fit
void step_kernel_coop(LEAD_PARAMS(T), StepParams<T> p) {
    step_body<T, Coop<MAXP>>(p, LEAD_OF(T));
}
// the cooperative form with a helper wave per workgroup (help_body): small
// scenes, whose body waves leave SIMDs idle
template <typename T, int MAXP>
__global__ __launch_bounds__(2 * STEP_BLOCK)
__attribute__((amdgpu_waves_per_eu(MAXP <= 16 ? RB_MIN_WAVES_COOP : 2)))
void step_kernel_coop_help(LEAD_PARAMS(T), StepParams<T> p) {
    step_body<T, CoopHelp<MAXP>>(p, LEAD_OF(T));
}
template <typename T, int MAXP>
__global__ __launch_bounds__(STEP_BLOCK)
#if RB_MIN_WAVES_G1 > 1
__attribute__((amdgpu_waves_per_eu(RB_MIN_WAVES_G1)))
#endif
void step_kernel_one(LEAD_PARAMS(T), StepParams<T> p) {
    step_body<T, One<MAXP>>(p, LEAD_OF(T));
}
// The box kernel (box worlds, after the step kernel): steps the bodies the
// step kernel deferred — those with a box-involved partner within bounding
// range — one lane per body with the box narrowphase (rb_boxes.hpp), from
// the same step-start data, so the step stays Jacobi across bodies.  One
// wave per SIMD: the narrowphase's registers fit without scratch, and the
// sphere step kernels keep their occupancy.
template <typename T, int MAXP>
__global__ __launch_bounds__(STEP_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1)))
void box_kernel(StepParams<T> p) {
    __shared__ int32_t s_id[MAXP * STEP_BLOCK];
    __shared__ T s_poly[48 * STEP_BLOCK];
    const int tid = threadIdx.x;
    const uint32_t gen = *p.cur.gen;
    const int32_t n = *p.defer_cnt;
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    // halo-exchanging shard: the peers' bounds, read with every lane active
    int32_t hb[6];
    const int64_t halo_e = p.halo.mail ? *p.halo.halo_e : 0;
    const bool halo = p.halo.mail && n > (int32_t)(blockIdx.x * STEP_BLOCK) && halo_bounds(p, halo_e, hb);
    for (int64_t qi0 = (int64_t)blockIdx.x * STEP_BLOCK; qi0 < n; qi0 += (int64_t)gridDim.x * STEP_BLOCK) {
        const int64_t qi = qi0 + tid;
        int32_t cell[6] = {INT32_MAX, 0, 0, 0, 0, 0};
        int32_t l = 0;
        // one lane per body: the lane's LDS column (partner list, polygon) is slot = tid
        if (qi < n) {
            l = p.defer_q[qi];
            // (of body_step's LDS arrays the box kernel has the list and the polygons; no helper, no epochs)
            body_step<T, BoxBody<MAXP>>(
                p, Lead<T>::of(p), true, l, tid, 0, tid, s_id, nullptr, nullptr, nullptr, nullptr, cell, gen, s_poly, nullptr,
                nullptr, nullptr, 0, nullptr, 0u);
        }
        if (halo) halo_push(p, halo_e, cell[0] != INT32_MAX, p.lo + l, cell, hb);   // (every lane of the wave)
        if (cell[0] != INT32_MAX)
#pragma unroll
            for (int d = 0; d < 3; ++d) { lo[d] = min(lo[d], cell[d]); hi[d] = max(hi[d], cell[d]); }
    }
    // halo exchange: the deferred bodies' new cells (the step kernel folded
    // only the bodies it stepped itself)
    if (p.bounds) fold_box(p.bounds, lo, hi);
    if (blockIdx.x == 0 && tid == 0) *p.defer_reset = 0;    // the next step's queue
}

// ---- split form (large scenes): search kernel + update kernel -------------
// The fused kernel's register footprint (the f64 solve) caps it at two
// waves per SIMD, too few to hide the search's dependent random loads.
// Split, the search runs at high occupancy and hands each body's sorted
// partner ids to the update through a per-slot list in HBM ([MAXP][S],
// coalesced by slot).
template <typename T, int MAXP, int G>
__global__ __launch_bounds__(STEP_BLOCK) void search_kernel(StepParams<T> p) {
    constexpr int NB = STEP_BLOCK / G;
    __shared__ int32_t s_id[MAXP * NB];
    __shared__ int32_t t_id[G > 1 ? MAXP * NB : 1];
    __shared__ Snap<T> s_pos[G > 1 ? MAXP * NB : 1];
    __shared__ Snap<T> t_pos[G > 1 ? MAXP * NB : 1];
    const int tid = threadIdx.x;
    const int slot = tid / G, k = tid % G;
    const int64_t lb = (int64_t)blockIdx.x * NB + slot;
    const bool active = lb < p.n_local;
    if (G == 1 && !active) return;
    const int32_t l = active ? (int32_t)lb : 0;
    const int32_t i = p.lo + l;
    const Snap<T> self = p.snap_cur[CHK(i, p.n_global)];
    const V3<T> x = {self.x, self.y, self.z};
    const int32_t kind = p.cs.kind[i];
    const T rad = p.cs.sx()[i];
    const uint32_t gen = *p.cur.gen;
    int32_t np_;
    bool defer = false;                          // split form: sphere worlds only
    if constexpr (G == 1) np_ = search_partners<T, MAXP, false>(p, i, kind, x, rad, self.r, s_id, tid, gen, defer);
    else np_ = search_coop<T, MAXP, G, false, -1>(p, active, i, kind, x, rad, self.r, s_id, s_pos, t_id, t_pos, slot, k, tid,
                                       gen, defer, [] {});
    if (!active) return;
    for (int s = k; s < np_; s += G) p.plist[CHK((int64_t)s * p.S + l, (int64_t)MAXP * p.S)] = s_id[s * NB + slot];
    if (k == 0) p.plist_cnt[CHK(l, p.S)] = np_;
}

template <typename T>
__global__ __launch_bounds__(STEP_BLOCK) void update_kernel(StepParams<T> p) {
    const int tid = threadIdx.x;
    const int64_t gt = (int64_t)blockIdx.x * STEP_BLOCK + tid;
    const int64_t lb = gt;
    int32_t cell[6] = {INT32_MAX, 0, 0, 0, 0, 0};
    const uint32_t gen_next = *p.cur.gen + 1u;
    const int64_t halo_e = p.halo.mail ? *p.halo.halo_e : 0;
    if (p.next.line && blockIdx.x == 0 && tid == 0) *p.next.gen = gen_next;
    if (lb < p.n_local) {
        const int32_t l = (int32_t)lb, i = p.lo + l;
        const Snap<T> self = p.snap_cur[CHK(i, p.n_global)];
        const V3<T> x = {self.x, self.y, self.z};
        const int32_t kind = p.cs.kind[i];
        const V3<T> sz = {p.cs.sx()[i], kind != 0 ? p.cs.sy()[i] : T(0), kind != 0 ? p.cs.sz()[i] : T(0)};
        const BodyIn<T> in = load_body(p, l, i);
        LazyInvI<T> invI;
        invI.I = in.I;
        invI.q = in.q;
        const int32_t np_ = p.plist_cnt[CHK(l, p.S)];
        if (RB_BOUNDS && np_ > 16) printf("RB_BOUNDS np_ %d at l %d\n", np_, l);
        body_update<T, FormTraits<SplitUpdate>::Update>(p, l, i, x, kind, sz, self.r, in, false, invI,
                                                        Partners<T>{np_, p.plist + l, p.S}, HelpDone{},
                                                        NextTable<T>{gen_next}, tid, cell, nullptr, 0);
    }
    if (p.bounds) fold_bounds(p.bounds, cell);
    if (p.halo.mail) {                           // halo-exchanging shard: push to the peers
        int32_t b[6];
        if (halo_bounds(p, halo_e, b)) halo_push(p, halo_e, cell[0] != INT32_MAX, (int32_t)(p.lo + lb), cell, b);
    }
}

template <typename T> hipError_t launch_step(const StepParams<T> &p, int maxp, int form, bool boxes, bool share, hipStream_t s) {
    const bool coop = form == FORM_COOP || form == FORM_COOP_HELP;
    const int nb = coop ? STEP_BLOCK / 8 : STEP_BLOCK;
    int64_t blocks = (p.n_local + nb - 1) / nb;
    if (blocks < 1) blocks = 1;
    const bool split = !coop && p.plist && !boxes;
    if (boxes && (!p.quat_cur || !p.defer_q || !p.defer_cnt || !p.defer_reset)) return hipErrorInvalidValue;
    // the cooperative search reads bucket slot snapshots: never launch it
    // on a table without them
    if (needs_slot_snapshots(coop, split) && (!p.cur.pos || (p.next.line && !p.next.pos))) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), one(STEP_BLOCK), two(2 * STEP_BLOCK);
    const bool m16 = maxp <= 16;
    if (split) {
        constexpr int GS = SPLIT_SEARCH_LANES;
        const dim3 sgrid((unsigned)(blocks * GS));
        pick([&](auto m) { hipLaunchKernelGGL((search_kernel<T, maxp_c(m.value), GS>), sgrid, one, 0, s, p); }, m16);
        hipLaunchKernelGGL((update_kernel<T>), grid, one, 0, s, p);
    } else if (form == FORM_COOP_HELP) {         // (box worlds: the box kernel follows)
        pick([&](auto m) { hipLaunchKernelGGL((step_kernel_coop_help<T, maxp_c(m.value)>), grid, two, 0, s, LEAD_ARGS(p), p); }, m16);
    } else if (coop) {
        pick([&](auto m) { hipLaunchKernelGGL((step_kernel_coop<T, maxp_c(m.value)>), grid, one, 0, s, LEAD_ARGS(p), p); }, m16);
    } else if (form == FORM_WIDE || form == FORM_WIDE_HELP) {
        const hipError_t we = launch_step_wide<T>(p, maxp, form == FORM_WIDE_HELP, share, s);
        if (we != hipSuccess) return we;
    } else {
        pick([&](auto m) { hipLaunchKernelGGL((step_kernel_one<T, maxp_c(m.value)>), grid, one, 0, s, LEAD_ARGS(p), p); }, m16);
    }
    if (boxes) {
        const int64_t bb = (p.n_local + STEP_BLOCK - 1) / STEP_BLOCK;
        const dim3 bgrid((unsigned)(bb < 1 ? 1 : bb > 256 ? 256 : bb));
        pick([&](auto m) { hipLaunchKernelGGL((box_kernel<T, maxp_c(m.value)>), bgrid, one, 0, s, p); }, m16);
    }
    return hipGetLastError();
}

#if RB_INST == 1
using Real = double;
#elif RB_INST == 2
using Real = float;
#else
#error "RB_INST: 1 (fp64) or 2 (fp32)"
#endif
template hipError_t launch_step<Real>(const StepParams<Real> &, int, int, bool, bool, hipStream_t);

}  // namespace rb
