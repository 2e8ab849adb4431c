// rb_step.hpp — the hot path on gfx950: the step-kernel body shared by the
// two step units (rb_step.hip: cooperative, one-lane, box and split forms;
// rb_step_wide.hip: the wide forms, built with their own scheduling flags).
// Device code only; included by those two units and, for candidate_hit, by
// the contact query (rb_world_contacts.hip), and nothing else.
//
// One launch per simulation step (rb::step_kernel), 64-thread workgroups
// (one wave):
//   K1 contact generation  — plane-sphere / plane-box corners against the
//      static planes; sphere-sphere against the step-start snapshot through
//      a spatial hash of cells (2 x 2 x 2 nearest cells).  Partners go to a
//      per-body list in LDS in ascending body id = the canonical
//      Gauss-Seidel order (SURVEY §7 hard part 1).  Small scenes search
//      cooperatively (8 lanes per body, one per cell), large ones one lane
//      per body.
//   K2 impulse solve       — per contact, in list order:
//      compute_collision_impulse_friction (collision.py:7-48) then
//      apply_impulse_friction (physics_utils.py:25-49);
//   K3 integrate           — x += v dt, q += 0.5 (0,w)*q dt, normalise
//      (collision.py:90-95): state written in place, the new position into
//      the next snapshot;
//   and the next step's broadphase: the body inserts its id into the next
//   table (a newer generation, rb_internal.hpp Table: nothing is cleared).
//   Two tables and two snapshots alternate, so a step reads only data no
//   thread of the same launch writes: Jacobi across bodies, exactly as
//   multi_sphere_bounce.py:43-46 (one mj_forward per step).
#pragma once

#include <type_traits>

#include "rb_device.hpp"

// diagnostic build only: per-wave s_memtime stamps at phase boundaries, into
// rb_stamp_buf, which the including unit defines first (rb_step_wide.hip:
// the host-side name of the buffer must be unique in the library)
#ifndef RB_STAMPS
#define RB_STAMPS 0
#endif
#if RB_STAMPS
#define STAMP(k)                                                                                  \
    do {                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        unsigned long long t_;                                                                    \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        /* a workgroup's second wave (shared search): its own buffer */                           \
        if ((threadIdx.x & 63) == 0 && blockIdx.x < (1u << 16))                                   \
            (threadIdx.x >> 6 ? rb_stamp_buf_help : rb_stamp_buf)[blockIdx.x][k] = t_;            \
        if (k == 0 || k == 6) { /* the constant-rate clock too, comparable across XCDs */            \
            unsigned long long r_;                                                                \
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r_)::"memory");        \
            /* (each wave in its own buffer: the shared search's second wave is the one that reaches 6) */ \
            if ((threadIdx.x & 63) == 0 && blockIdx.x < (1u << 16))                               \
                (threadIdx.x >> 6 ? rb_stamp_buf_help : rb_stamp_buf)[blockIdx.x][k == 0 ? 12 : 13] = r_; \
        }                                                                                         \
    } while (0)
#else
#define STAMP(k) do {} while (0)
#endif

#include "rb_boxes.hpp"
#include "rb_grid.hpp"
#include "rb_halo.hpp"
#include "rb_internal.hpp"
#include "rb_body.hpp"

// diagnostic builds only (scripts/ablate.py): 1 = skip the sphere-sphere
// broadphase, 2 = skip the world-inertia inverse (identity), 3 = empty
// kernel (launch floor), 4 = search only (no body update), 0 = product
#ifndef RB_ABLATE
#define RB_ABLATE 0
#endif

namespace rb {

// Candidate test shared by every search form: true if the candidate with
// snapshot s and tagged id tj is a partner of body i — for two spheres the
// sphere-sphere contact test, for a box-involved pair overlapping bounding
// spheres (the narrowphase then decides; oracle gen_contacts does the
// same).  Only the box kernel (BOXES) takes such a pair; the sphere step
// kernels mark the body deferred to it (box worlds, sharded or not: p.defer_q;
// a sharded world's exchange carries the boxes' orientations).
template <typename T, bool BOXES>
__device__ __forceinline__ bool candidate_hit(const StepParams<T> &p, int32_t i, int32_t kind, V3<T> x, T rad, T bi,
                                              uint32_t tj, const Snap<T> &s, bool &defer) {
    const int32_t j = (int32_t)(tj & ~BOX_FLAG);
    if (j == i) return false;
    const V3<T> cj = {s.x, s.y, s.z};
    if (kind != 0 || (tj & BOX_FLAG)) {
        const V3<T> dd = {x.x - cj.x, x.y - cj.y, x.z - cj.z};
        const bool near = sqroot(mj_dot(dd, dd)) <= bi + s.r;
        if (BOXES) return near;
        if (near) {
            if (p.defer_q) defer = true;
            else atomicOr(p.err, ERR_UNSUPPORTED);
        }
        return false;
    }
    return sphere_sphere_hit(x, rad, cj, s.r);
}

// K1, one lane per body (rb_grid.hpp search_buckets with the main law's
// candidate test).
template <typename T, int MAXP, bool BOXES>
__device__ __forceinline__ int32_t search_partners(const StepParams<T> &p, int32_t i, int32_t kind, V3<T> x,
                                                   T rad, T bi, int32_t *s_id, int tid, uint32_t gen, bool &defer) {
    // the box kernel also runs in cooperative worlds (a hash per cell)
    constexpr int L = BOXES ? LAYOUT_ANY : LAYOUT_LINEAR;
    return search_buckets<T, MAXP, L>(p, i, x, s_id, tid, gen, [&](uint32_t tj, const Snap<T> &s) {
        return candidate_hit<T, BOXES>(p, i, kind, x, rad, bi, tj, s, defer);
    });
}

// K1, wide one-lane form (rb_grid.hpp search_buckets_wide)
template <typename T, int MAXP, bool BOXES, bool EP, typename Overlap>
__device__ __forceinline__ int32_t search_partners_wide(const StepParams<T> &p, int32_t i, int32_t kind, V3<T> x,
                                                        T rad, T bi, int32_t *s_id, uint32_t *s_cand, uint8_t *s_didx,
                                                        Snap<T> *s_hpos, int tid, uint32_t gen, const Table<T> &cur,
                                                        bool appended, uint32_t &b0, bool &defer, Overlap overlap) {
    return search_buckets_wide<T, MAXP, EP>(
        p, i, x, s_id, s_cand, s_didx, s_hpos, tid, gen, cur, appended, b0,
        [&](uint32_t tj, const Snap<T> &s) { return candidate_hit<T, BOXES>(p, i, kind, x, rad, bi, tj, s, defer); },
        overlap);
}

// K1 for small scenes: G lanes per body, lane k of the group owns neighbour
// cell k.  Its header (count, first 2 ids) and first RB_QSPEC slot snapshots are
// loaded together (slots past the count are stale and ignored), and while
// they are in flight the lane evaluates the body's inverse world inertia
// (pre, if PRE).  Hits become a bitmask over the bucket slots; a group prefix sum
// (shuffles) places them — id and snapshot — in LDS, and the group
// rank-sorts them by body id into s_id / s_pos.  Same contact set and order
// as search_partners.
template <typename T, int MAXP, int G, bool BOXES, int RL, typename Overlap>
__device__ __forceinline__ int32_t search_coop(const StepParams<T> &p, bool active, int32_t i, int32_t kind,
                                               V3<T> x, T rad, T bi, int32_t *s_id, Snap<T> *s_pos, int32_t *t_id,
                                               Snap<T> *t_pos, int slot, int k, int lane, uint32_t gen,
                                               bool &defer, Overlap overlap) {
    static_assert(G == 8, "one lane per neighbour cell");
    constexpr int NB = STEP_BLOCK / G;
    constexpr int QB = RB_QBATCH;
    constexpr int QS = RB_QSPEC;                 // slots loaded before the count is known
    int32_t cx = 0, cy = 0, cz = 0, sx = 1, sy = 1, sz = 1;
    bool ok = active;
    if (active && !neighbourhood(p, x, cx, cy, cz, sx, sy, sz)) {
        if (k == 0) atomicOr(p.err, ERR_DOMAIN);
        ok = false;
    }
    const uint32_t b = bucket_of(cx + ((k & 1) ? sx : 0), cy + ((k & 2) ? sy : 0), cz + ((k & 4) ? sz : 0),
                                 p.grid);
    const int64_t base = (int64_t)b * LINE_WORDS;      // slot snapshots: slot s at base + s
    [[maybe_unused]] const int tid = lane;   // STAMP
    STAMP(8);
    // loaded unconditionally (b is a valid bucket for every lane) and the
    // count clamped only after overlap(): a use inside a branch would make
    // the wave wait for the loads before that work starts
    const int rl = RL >= 0 ? RL : grid_rl(p.grid.super);   // heads per line: cooperative worlds 1 (rb_api_world.hip)
    const uint4 id4 = bucket_head(p.cur, b, rl);
    Snap<T> p4[QS > 0 ? QS : 1];                  // (RB_QSPEC=0: a diagnostic build)
#pragma unroll
    for (int u = 0; u < QS; ++u) p4[u] = p.cur.pos[base + u];
    __builtin_amdgcn_sched_barrier(0);            // the bucket loads issue before the body work
    overlap();                                    // body work under the bucket loads
    int32_t c = !ok ? 0 : head_count(id4, gen);
    STAMP(9);
    const int gbase = lane & ~(G - 1);
#pragma unroll
    for (int j = 0; j < G; ++j) {
        const uint32_t bj = (uint32_t)__shfl((int)b, gbase + j);
        if (j < k && bj == b) c = 0;                  // bucket already visited by a lower cell
    }
    uint32_t mask = 0;
#pragma unroll
    for (int u = 0; u < QS; ++u)
        if (u < c && candidate_hit<T, BOXES>(p, i, kind, x, rad, bi, bucket_id(p.cur, b, id4, u, rl), p4[u], defer)) mask |= 1u << u;
    for (int s0 = QS; s0 < c; s0 += QB) {
        uint32_t tj[QB];
        Snap<T> sn[QB];
#pragma unroll
        for (int u = 0; u < QB; ++u) {
            if (s0 + u >= c) break;                   // stay inside this bucket's slots
            tj[u] = bucket_id(p.cur, b, id4, s0 + u, rl);
            sn[u] = p.cur.pos[base + s0 + u];
        }
#pragma unroll
        for (int u = 0; u < QB; ++u)
            if (s0 + u < c && candidate_hit<T, BOXES>(p, i, kind, x, rad, bi, tj[u], sn[u], defer)) mask |= 1u << (s0 + u);
    }
    // rare: ids past a full bucket (rb_grid.hpp spill_scan), counted here,
    // placed after the slot hits below (id-indexed snapshots: no slot copy)
    int32_t hs = 0;
    const bool spl = c > 0 && head_spilled(id4, gen);
    if (spl)
        spill_scan(p.cur, gen, b, [&](uint32_t t) {
            if (candidate_hit<T, BOXES>(p, i, kind, x, rad, bi, t, p.snap_cur[CHK(t & ~BOX_FLAG, p.n_global)], defer)) ++hs;
        });
    STAMP(10);
    if (p.defer_q) {                              // any lane of the group: the body is deferred
        int dv = defer ? 1 : 0;
        dv |= __shfl_xor(dv, 1);
        dv |= __shfl_xor(dv, 2);
        dv |= __shfl_xor(dv, 4);
        defer = dv != 0;
    }
    const int h = __popc(mask) + hs;
    int pre_n = 0, total = 0;
#pragma unroll
    for (int j = 0; j < G; ++j) {
        const int hj = __shfl(h, gbase + j);
        total += hj;
        if (j < k) pre_n += hj;
    }
    if (total > MAXP && k == 0) atomicOr(p.err, ERR_PARTNER_OVERFLOW);
    int o = pre_n;
#pragma unroll
    for (int u = 0; u < QS; ++u) {
        if (!((mask >> u) & 1u)) continue;
        if (o < MAXP) {
            t_id[slot * MAXP + o] = (int32_t)(bucket_id(p.cur, b, id4, u, rl) & ~BOX_FLAG);
            t_pos[slot * MAXP + o] = p4[u];
        }
        ++o;
    }
    for (uint32_t rest = mask & ~((1u << QS) - 1u); rest; rest &= rest - 1) {
        const int sl = __builtin_ctz(rest);
        if (o < MAXP) {                               // re-read: L1-hot from the batch above
            t_id[slot * MAXP + o] = (int32_t)(bucket_id(p.cur, b, id4, sl, rl) & ~BOX_FLAG);
            t_pos[slot * MAXP + o] = p.cur.pos[base + sl];
        }
        ++o;
    }
    if (hs)
        spill_scan(p.cur, gen, b, [&](uint32_t t) {
            const Snap<T> sn = p.snap_cur[CHK(t & ~BOX_FLAG, p.n_global)];
            bool d2 = false;
            if (!candidate_hit<T, BOXES>(p, i, kind, x, rad, bi, t, sn, d2)) return;
            if (o < MAXP) {
                t_id[slot * MAXP + o] = (int32_t)(t & ~BOX_FLAG);
                t_pos[slot * MAXP + o] = sn;
            }
            ++o;
        });
    __syncthreads();
    STAMP(11);
    const int tot = total < MAXP ? total : MAXP;
    for (int qq = k; qq < tot; qq += G) {
        const int32_t id = t_id[slot * MAXP + qq];
        int r = 0;
        for (int j = 0; j < tot; ++j) r += t_id[slot * MAXP + j] < id;
        s_id[r * NB + slot] = id;
        s_pos[r * NB + slot] = t_pos[slot * MAXP + qq];
    }
    __syncthreads();
    return tot;
}

// Per-body inputs of K2, loaded by the cooperative form before the search
// (their latency hides under it) and by the one-lane form after it (fewer
// registers live across the search).
template <typename T> struct BodyIn {
    Q4<T> q;
    V3<T> v, w;
    T m;
    V3<T> I;
};
template <typename T>
__device__ __forceinline__ BodyIn<T> load_body(const BodyState<T> &st, const BodyConsts<T> &cs, int32_t l, int32_t i) {
    BodyIn<T> b;
    b.q = {st.qw()[l], st.qx()[l], st.qy()[l], st.qz()[l]};
    b.v = {st.vx()[l], st.vy()[l], st.vz()[l]};
    b.w = {st.wx()[l], st.wy()[l], st.wz()[l]};
    // diagnostic (RB_ABLATE 8): every body reads body 0's constants (a
    // scene of identical bodies stays bit-exact) — the cost of the per-body
    // constant loads
    const int32_t ci = RB_ABLATE == 8 ? 0 : i;
    b.m = cs.mass()[ci];
    b.I = {cs.ix()[ci], cs.iy()[ci], cs.iz()[ci]};
    return b;
}
template <typename T> __device__ __forceinline__ BodyIn<T> load_body(const StepParams<T> &p, int32_t l, int32_t i) {
    return load_body(p.st, p.cs, l, i);
}

// The fields a step's first loads need (the body's snapshot, kind, state and
// constants).  The step kernels take them as leading scalar arguments, which
// gfx950 preloads into SGPRs as the waves launch (the units are built with
// -amdgpu-kernarg-preload-count), so their first loads wait for no scalar
// load of the parameter block (measured 0.27 us per launch in
// scripts/preload_probe.hip); the box kernel takes them from the block.
// 14 dwords: the preload budget beside the two of the kernarg pointer.
//
// The instances of worlds with append epochs (the _ep kernels of
// rb_step_wide.hip) take LEAD_EP_*: the address of the lead block's
// generation word as well (gen_cur, lead_words below), for which the row
// strides (st.S, cs.Npad) travel as 32-bit values — they count bodies, as
// n_local and lo do; cs.kind stays a pointer (an allocation of its own, at no
// fixed distance from cs.base).  Every other instance keeps LEAD_* and reads
// its generation through the parameter block (body_step): there the early
// read lost (C2, cooperative form: 6.98 -> 7.13 us per step; C5: 8.72 -> 9.18)
template <typename T> struct Lead {
    const Snap<T> *snap_cur;
    BodyState<T> st;
    BodyConsts<T> cs;
    int32_t n_local, lo;
    const uint32_t *gen_cur = nullptr; // _ep kernels: p.cur.gen, gen[step parity] of the lead block (rb_internal.hpp)
    __device__ static Lead of(const StepParams<T> &p) { return Lead{p.snap_cur, p.st, p.cs, p.n_local, p.lo}; }
};
#define LEAD_PARAMS(T)                                                                                            \
    const Snap<T> *snap_cur, T *st_base, int64_t st_S, const T *cs_base, int64_t cs_Npad, const int32_t *cs_kind, \
        int32_t n_local, int32_t lo
#define LEAD_OF(T)                                                                                                \
    Lead<T> { snap_cur, BodyState<T>{st_base, st_S}, BodyConsts<T>{cs_base, cs_Npad, cs_kind}, n_local, lo }
#define LEAD_ARGS(p) (p).snap_cur, (p).st.base, (p).st.S, (p).cs.base, (p).cs.Npad, (p).cs.kind, (p).n_local, (p).lo
#define LEAD_EP_PARAMS(T)                                                                                         \
    const Snap<T> *snap_cur, T *st_base, const T *cs_base, const int32_t *cs_kind, const uint32_t *gen_cur,       \
        int32_t st_S, int32_t cs_Npad, int32_t n_local, int32_t lo
#define LEAD_EP_OF(T)                                                                                             \
    Lead<T> { snap_cur, BodyState<T>{st_base, st_S}, BodyConsts<T>{cs_base, cs_Npad, cs_kind}, n_local, lo, gen_cur }
#define LEAD_EP_ARGS(p)                                                                                           \
    (p).snap_cur, (p).st.base, (p).cs.base, (p).cs.kind, (p).cur.gen, (int32_t)(p).st.S, (int32_t)(p).cs.Npad, (p).n_local, (p).lo

// The lead block's words of this step: its table's generation and its epoch
// control word, with ONE scalar load of the block, issued from preloaded
// SGPRs — beside the parameter block's scalar loads, not behind them, and
// behind no vector load.  gen_cur points at gen[sp] inside the 16-byte-aligned
// block, so the block's address and the step's parity sp both come from it.
// Why a scalar (constant address space) read is sound: the step of parity sp
// reads only gen[sp] and ctrl[sp], and no thread of the same launch writes
// those — block 0 writes gen[1 - sp] and ctrl[1 - sp] (step_body's tail),
// words this step never looks at; every writer between launches (prime(),
// the step before) is ordered before this launch on the stream.
struct LeadWords { uint32_t gen, ctrl; };
typedef uint32_t lead_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ LeadWords lead_words(const uint32_t *gen_cur) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(gen_cur);
    const lead_u32x4 b = *(const __attribute__((address_space(4))) lead_u32x4 *)(a & ~uintptr_t(4 * LEAD_WORDS - 1));
    const bool odd = (a & 4u) != 0;
    static_assert(LEAD_GEN == 0 && LEAD_CTRL == 2 && LEAD_WORDS == 4, "the block's layout");
    return LeadWords{odd ? b.y : b.x, odd ? b.w : b.z};
}

#ifndef RB_SOLVE_PIPE
#define RB_SOLVE_PIPE 1
#endif
// shared search, the helper wave's own work: 0: all of it under its head
// loads; 1: inv(I_w) there, gravity and the plane contacts under its first
// candidate batch
// (measured with RB_SHARE_SPLIT, rb_grid.hpp: only the two together pay)
#ifndef RB_SHARE_WORK2
#define RB_SHARE_WORK2 1
#endif
// ... of the MAXP 32 instances (with RB_SHARE_SPLIT32)
#ifndef RB_SHARE_WORK2_32
#define RB_SHARE_WORK2_32 0
#endif
// shared search: the helper wave finishes the body (merge, solves,
// integration, insert, the kernel's tail) from its own registers and the body
// wave only searches.  Not in the MAXP 32 instances — worlds made for piles,
// C4: there the move alone lost, 37.6 -> 38.4 us per step
// (profiles/help_finish/variants_c4_ab.log) — which keep the hand-over in
// LDS to the body wave
#ifndef RB_SHARE_FINISH32
#define RB_SHARE_FINISH32 0
#endif
template <int MAXP> constexpr bool share_finish() { return MAXP <= 16 || RB_SHARE_FINISH32 != 0; }
// batches of partner snapshots in flight ahead of the solve (the helper-wave
// wide form only: its register budget has room for a second batch)
#ifndef RB_SOLVE_DEPTH
#define RB_SOLVE_DEPTH 1
#endif

// ---- a step kernel's form ---------------------------------------------------
// step_body and body_step take one type F that names the form: a struct of
// the flags below, every one with a default here.  The forms that exist are
// the structs after it; a call site names one of them.  A form holds only what
// body_step depends on (HALO is step_body's own parameter), and body_update
// takes the smaller UpdateForm: kernels that agree in what a function sees
// share one instance of it, as they always did — with an instance per kernel
// the wide unit's instructions come out in another order
// (profiles/step_forms/README.md).
struct FormDefaults {
    static constexpr int G = 1;            // lanes per body: 1, or 8 (the cooperative search, one per neighbour cell)
    // the one-lane form for one wave per SIMD (search_buckets_wide; state
    // loads and inv(I_w) under the head loads)
    static constexpr bool WIDE = false;
    static constexpr bool BOXES = false;   // the box kernel's body: box-involved pairs and their narrowphase
    static constexpr bool HELP = false;    // a helper wave per workgroup (help_body)
    static constexpr bool EP = false;      // worlds with append epochs (the _ep kernels; rb_internal.hpp Epoch)
    // SHARE: the helper wave of the wide form also searches half of each body's
    // neighbourhood (body_step; rb_grid.hpp search_half_wide) and then finishes
    // the body — merge, solves, integration, insert and step_body's tail —
    // from its own registers; the body wave only searches
    static constexpr bool SHARE = false;
    // the lead is preloaded (step_body's callers); false only for the box
    // kernel's call of body_step, which takes it from the parameter block
    static constexpr bool PRE = true;
};
template <int M> struct One : FormDefaults { static constexpr int MAXP = M; };
template <int M> struct Coop : One<M> { static constexpr int G = 8; };
template <int M> struct CoopHelp : Coop<M> { static constexpr bool HELP = true; };
template <int M> struct Wide : One<M> { static constexpr bool WIDE = true; };
template <int M, bool S> struct WideHelp : Wide<M> { static constexpr bool HELP = true, SHARE = S; };
template <int M> struct WideEp : Wide<M> { static constexpr bool EP = true; };
template <int M, bool S> struct WideHelpEp : WideHelp<M, S> { static constexpr bool EP = true; };
template <int M> struct BoxBody : One<M> { static constexpr bool BOXES = true, PRE = false; };
struct SplitUpdate : One<32> {};             // the split form's update_kernel (body_update alone, its list in HBM)

// body_update's form — the partner mode, the box narrowphase, the solve
// depth, the epochs' crowding flag — and what follows from it
template <int PM_, bool BOXES_, int SD_, bool EP_> struct UpdateForm {
    static constexpr int PM = PM_, SD = SD_;
    static constexpr bool BOXES = BOXES_, EP = EP_;
    // sphere kernels (RB_SOLVE_PIPE): the next batch's snapshots load under
    // this batch's solves — a body with many partners (C4's pile-ups: up to
    // 28) otherwise waits one round trip per batch of partners re-read from memory
    static constexpr bool PIPE = !BOXES && RB_SOLVE_PIPE && PM != 1;   // (the cooperative form: LDS only)
    static constexpr bool DEEP = PIPE && SD > 1;
    // the next table's insert.  The one-lane and wide forms (and the split
    // form's update) run in linear-layout worlds only; the cooperative form
    // and the box kernel read the layout
    static constexpr int L = (PM == 2 || (PM == 0 && !BOXES)) ? LAYOUT_LINEAR : LAYOUT_ANY;
    // heads per line: known in the cooperative and wide forms (rb_api_world.hip)
    static constexpr int RL = PM == 1 ? 0 : PM == 2 ? 2 : -1;
};
// What follows from a form, and which forms there are.
template <typename F> struct FormTraits {
    static_assert(F::G == 1 || F::G == 8, "one lane per body, or one per neighbour cell");
    static_assert(!F::SHARE || (F::G == 1 && F::WIDE && F::HELP && !F::BOXES), "shared search: the helper-wave wide form");
    static_assert(!F::EP || (F::PRE && F::WIDE), "append epochs: the wide step kernels");
    static_assert(!F::HELP || !F::BOXES, "helper waves: the sphere step kernels");
    static constexpr int NB = STEP_BLOCK / F::G;          // bodies per workgroup
    // state loads issued before the search (the wide form measured 5 % slower
    // with them issued after the bucket heads, C3)
    static constexpr bool EARLY = F::G > 1 || F::WIDE;
    // worlds with epochs, shared search: the kind-dependent selects of
    // body_step are made under the head loads (late_kind, called by the
    // search's overlap): the wait for kind, sy and sz counts loads in issue
    // order, so ahead of the heads it would hold them back until the
    // finishing wave's state loads, issued after these, had landed
    static constexpr bool LATE = F::SHARE && F::EP;
    // shared search: the helper wave finishes the body (share_finish above)
    static constexpr bool FIN = F::SHARE && share_finish<F::MAXP>();
    // shared search, the helper wave's gravity and plane contacts under its
    // first candidate batch (RB_SHARE_WORK2 above; not with applied forces:
    // body_update's)
    static constexpr bool WORK2 = F::MAXP > 16 ? RB_SHARE_WORK2_32 != 0 : RB_SHARE_WORK2 != 0;
    // body_update's: the partner mode (Partners below) and the batches of
    // partner snapshots ahead of the solve (RB_SOLVE_DEPTH above)
    static constexpr int PM = F::G > 1 ? 1 : (F::WIDE && RB_WIDE_LDSPOS) ? 2 : 0;
    static constexpr int SD = (F::WIDE && F::HELP) ? RB_SOLVE_DEPTH : 1;
    // what body_update depends on: the forms that agree in it share one instance
    using Update = UpdateForm<PM, F::BOXES, SD, F::EP>;
};

// body_update's inputs beside the body itself.
// The sorted partner list: n ids at id[u * stride] (an LDS column, or the
// split form's per-slot list in HBM); snapshots (PM, partner mode) at
// pos[u * stride] (LDS, PM = 1: cooperative form), at pos[d * stride] for
// the discovery index d = didx[u * stride] < WIDE_HPOS (LDS, PM = 2: wide
// form) or gathered from the step-start snapshot (PM = 0, and PM = 2 past
// WIDE_HPOS).  PM is a template flag, so LDS accesses stay ds_read (no flat loads).
template <typename T> struct Partners {
    int32_t n;
    const int32_t *id;
    int64_t stride;
    const Snap<T> *pos = nullptr;
    const uint8_t *didx = nullptr;
};
// what a helper wave has done for the body already (help_body): its plane
// contacts, nrec of them recorded
struct HelpDone {
    int32_t nrec = 0;
    bool planes = false;
};
// the next step's table: the generation the body inserts with; tab: the table
// chosen by the step's epoch control word (body_step), else p.next; keep:
// append steps, the bucket that lists the body already — a body still in it
// claims and publishes nothing
template <typename T> struct NextTable {
    uint32_t gen;
    const Table<T> *tab = nullptr;
    uint32_t keep = NO_BUCKET;
};

// Everything after the contact search for one body (lane): gravity (unless
// already applied: forced), the Gauss-Seidel solves in canonical order,
// integration, next-step insert.  poly, ps: the box kernel's clipping
// polygon column in LDS and its stride (BOXES).
template <typename T, typename U>
__device__ __forceinline__ void body_update(const StepParams<T> &p, int32_t l, int32_t i, V3<T> x, int32_t kind,
                                            V3<T> sz, T bi, const BodyIn<T> &in, bool forced, LazyInvI<T> &invI,
                                            const Partners<T> &pa, const HelpDone &help, const NextTable<T> &nx,
                                            int tid, int32_t *cell, T *poly, int ps) {
    constexpr int PM = U::PM;
    constexpr bool BOXES = U::BOXES, EP = U::EP;
    const int32_t np_ = pa.n;
    const Q4<T> q = in.q;
    V3<T> v = in.v;
    V3<T> w = in.w;
    const T m = in.m;

    // ---- a4: gravity / applied force (collision.py:66-70) ------------------
    if (!forced) apply_force(p, l, m, invI, v, w);
    const T k = impulse_k(m);

    STAMP(3);
    int32_t nrec = help.nrec;
    // ---- K2: plane contacts, plane order -------------------------------------
    // (a sphere's already solved by the helper wave when help.planes)
    if (kind == 0 && !help.planes) solve_planes_sphere(p, p, l, x, sz.x, m, k, invI, v, w, nrec);
    M3<T> M;                                       // box orientation (mj_kinematics of the free joint)
    if (kind != 0) M = mj_body_mat(q);             // (the box narrowphase below needs it too)
    if (kind != 0 && !help.planes) solve_planes_box(p, p, l, x, M, sz, m, k, invI, v, w, nrec);

    // ---- K2: sphere partners in ascending id order ---------------------------
    // (partner snapshots fetched PB at a time; the solve itself is the
    // reference's sequential Gauss-Seidel).  The box kernel takes them one at
    // a time: each unrolled copy of the loop body inlines the box
    // narrowphase (4 copies made the kernel 169 KB)
    constexpr int PB = BOXES ? 1 : 4;
    auto fetch = [&](int s0, int32_t (&jj)[PB], Snap<T> (&pe)[PB]) {
#pragma unroll
        for (int u = 0; u < PB; ++u)
            if (s0 + u < np_) jj[u] = pa.id[CHK((s0 + u) * pa.stride, 32 * pa.stride)];
#pragma unroll
        for (int u = 0; u < PB; ++u) {
            if (s0 + u >= np_) continue;
            if constexpr (PM == 1) {
                pe[u] = pa.pos[(s0 + u) * pa.stride];
            } else if constexpr (PM == 2) {
                const int d = pa.didx[(s0 + u) * pa.stride];
                pe[u] = d < WIDE_HPOS ? pa.pos[d * pa.stride] : xld(p.snap_cur + CHK(jj[u], p.n_global));
            } else {
                pe[u] = xld(p.snap_cur + CHK(jj[u], p.n_global));
            }
        }
    };
    // the next batch, or two, in flight under this batch's solves (UpdateForm PIPE, DEEP)
    [[maybe_unused]] int32_t jn[PB], jn2[PB];
    [[maybe_unused]] Snap<T> sn_next[PB], sn_next2[PB];
    constexpr bool pipe = U::PIPE, deep = U::DEEP;
    if constexpr (pipe) {
        if (np_ > 0) fetch(0, jn, sn_next);
        if constexpr (deep)
            if (np_ > PB) fetch(PB, jn2, sn_next2);
    }
    for (int s0 = 0; s0 < np_; s0 += PB) {
        int32_t jj[PB];
        Snap<T> pe[PB];
        if constexpr (deep) {
#pragma unroll
            for (int u = 0; u < PB; ++u) {
                jj[u] = jn[u]; pe[u] = sn_next[u];
                jn[u] = jn2[u]; sn_next[u] = sn_next2[u];
            }
            if (s0 + 2 * PB < np_) fetch(s0 + 2 * PB, jn2, sn_next2);
        } else if constexpr (pipe) {
#pragma unroll
            for (int u = 0; u < PB; ++u) { jj[u] = jn[u]; pe[u] = sn_next[u]; }
            if (s0 + PB < np_) fetch(s0 + PB, jn, sn_next);
        } else {
            fetch(s0, jj, pe);
        }
#pragma unroll
        for (int u = 0; u < PB; ++u) {
            if (s0 + u >= np_) break;
            const int32_t j = jj[u];
            const V3<T> cj = {pe[u].x, pe[u].y, pe[u].z};
            const T rj = pe[u].r;
            if constexpr (BOXES) {
                const int32_t kj = p.cs.kind[j];
                if (kind != 0 || kj != 0) {
                    // box-involved pair (rb_boxes.hpp), from step-start data of both
                    // bodies, in MuJoCo's geom order: sphere before box, boxes by id
                    auto emit = [&](const Contact<T> &con, int ck, bool self_g1) {
                        record(p, l, nrec, j, ck, con.dist);
                        const V3<T> n = (p.oriented && self_g1) ? V3<T>{-con.frame.x, -con.frame.y, -con.frame.z}
                                                                : con.frame;
                        solve_contact(p, con, x, n, m, k, invI, v, w);
                    };
                    M3<T> Mj;
                    const V3<T> hj = {p.cs.sx()[j], p.cs.sy()[j], p.cs.sz()[j]};
                    if (kj != 0) {
                        const T *qj = p.quat_cur + 4 * (int64_t)j;
                        Mj = mj_body_mat(Q4<T>{qj[0], qj[1], qj[2], qj[3]});
                    }
                    // geom1: the sphere of a sphere-box pair, else the lower id
                    // (one call of each primitive, operands selected)
                    const bool g1 = (kind == 0 && kj != 0) || (kind != 0 && kj != 0 && i < j);
                    const V3<T> p1 = g1 ? x : cj, p2 = g1 ? cj : x;
                    const V3<T> h1 = g1 ? sz : hj, h2 = g1 ? hj : sz;
                    M3<T> M1, M2;
#pragma unroll
                    for (int k = 0; k < 9; ++k) { M1.a[k] = g1 ? M.a[k] : Mj.a[k]; M2.a[k] = g1 ? Mj.a[k] : M.a[k]; }
                    if (kind == 0 || kj == 0) {
                        Contact<T> con;
                        if (sphere_box(p1, g1 ? sz.x : rj, p2, M2, h2, con)) emit(con, CK_SPHERE_BOX, g1);
                    } else {
                        box_box(p1, M1, h1, p2, M2, h2, poly, ps,
                                [&](const Contact<T> &c, int ck) { emit(c, ck, g1); });
                    }
                    continue;
                }
            }
            solve_sphere_pair(p, l, i, j, x, sz.x, cj, rj, m, k, invI, v, w, nrec);
        }
    }
    if (p.rec_count) p.rec_count[l] = nrec;
    STAMP(4);

    // ---- K3: integrate (collision.py:90-100) ---------------------------------
    if (p.bounds) {                              // peer-to-peer exchange: the step-start cell too
        int32_t cx, cy, cz;
        if (cell_of(x.x, x.y, x.z, p.grid.inv_cs, cx, cy, cz)) { cell[3] = cx; cell[4] = cy; cell[5] = cz; }
    }
    integrate_position(x, v, p.dt);
    Snap<T> sn;
    sn.x = x.x; sn.y = x.y; sn.z = x.z; sn.r = bi;
    // next step's broadphase: the slot atomic goes first (a later load or
    // atomic would wait for every older store), its round trip overlaps the
    // snapshot store and the quaternion update
    Claim cl{0u, 0, 0ull, 0u, 0};
    constexpr int L = U::L, RL = U::RL;         // the insert's layout and heads per line
    const Table<T> &next = nx.tab ? *nx.tab : p.next;
    if (next.line) cl = claim_slot<L, RL>(p.grid, next, p.err, sn, nx.gen, nx.keep);
    wt_store(p.snap_next + i, sn);
    if (p.bounds) {                              // peer-to-peer exchange: this body's new cell
        int32_t cx, cy, cz;
        if (cell_of(sn.x, sn.y, sn.z, p.grid.inv_cs, cx, cy, cz)) { cell[0] = cx; cell[1] = cy; cell[2] = cz; }
    }
    STAMP(5);
    Q4<T> qn;
    integrate_orientation(qn, q, w, p.dt);
    wt_store(p.st.vx() + l, v.x); wt_store(p.st.vy() + l, v.y); wt_store(p.st.vz() + l, v.z);
    wt_store(p.st.wx() + l, w.x); wt_store(p.st.wy() + l, w.y); wt_store(p.st.wz() + l, w.z);
    wt_store(p.st.qw() + l, qn.w); wt_store(p.st.qx() + l, qn.x); wt_store(p.st.qy() + l, qn.y);
    wt_store(p.st.qz() + l, qn.z);
    // next step's orientation snapshot (box worlds), from every kernel that
    // steps a box: the box kernel reads it for a partner that was out of any
    // box pair's range (stepped by a sphere kernel) in the step before
    if (p.quat_next && kind != 0) {
        T *qs = p.quat_next + 4 * (int64_t)i;
        wt_store(qs + 0, qn.w); wt_store(qs + 1, qn.x); wt_store(qs + 2, qn.y); wt_store(qs + 3, qn.z);
    }
    publish_slot<RL>(next, p.err, cl, sn, (uint32_t)i | (kind != 0 ? BOX_FLAG : 0u));
    // worlds with append epochs: a claim past the bucket's head — by an
    // appender, or by any body of a rebuild step (a pile: the table starts
    // crowded) — raises the crowding flag; block 0 of the next step reads
    // it and cuts the epoch short (step_body).  A plain store by one lane
    // per wave: every writer stores the same word, so no atomic is needed
    // (a pile raises it from a thousand waves per step)
    if constexpr (EP) {
        {
            const bool past = cl.ok && (uint32_t)(cl.old >> 32) == cl.gen && (uint32_t)cl.old >= (uint32_t)WIDE_HEAD_IDS;
            const unsigned long long m = __ballot(past);
            if (past && (int)(threadIdx.x & 63) == __ffsll(m) - 1) *p.ep.crowd = 1;
        }
    }
    STAMP(6);
}

// The helper wave's hand-over to the body wave through LDS: one record per
// body in column layout (row r of body h at o[r * NB], o = base + h), written
// by help_body and by the helper wave of the MAXP 32 shared search, read by
// body_step.  Rows: inv(I_w) 9, v 3, w 3, the recorded plane contacts 1
// (HELP_NO_PLANES: the planes are not solved), q 4, m 1.  (The three places
// index the rows in line: a store or load function of the record changes the
// wide unit's instruction order, profiles/step_forms/README.md)
enum : int { HELP_INVI = 0, HELP_V = 9, HELP_W = 12, HELP_NREC = 15, HELP_Q = 16, HELP_M = 20, HELP_REALS = 21 };
constexpr int HELP_NO_PLANES = -1;

// One body (G lanes): contact search, then (lane 0) the update.  WIDE: the
// one-lane form for one wave per SIMD (search_buckets_wide; state loads and
// inv(I_w) under the head loads).
template <typename T, typename F>
__device__ __forceinline__ void body_step(const StepParams<T> &p, const Lead<T> &ld, bool active, int64_t lb, int slot,
                                          int k, int tid,
                                          int32_t *s_id, Snap<T> *s_pos, int32_t *t_id, Snap<T> *t_pos,
                                          uint32_t *s_cand, int32_t *cell, uint32_t gen, T *s_poly,
                                          uint8_t *s_didx, Snap<T> *s_hpos, T *s_help, int role, uint32_t *s_half,
                                          uint32_t ctrl /* PRE && EP: the step's epoch control word */) {
    using FT = FormTraits<F>;
    constexpr int MAXP = F::MAXP, G = F::G, NB = FT::NB;
    constexpr bool WIDE = F::WIDE, BOXES = F::BOXES, PRE = F::PRE, HELP = F::HELP, EP = F::EP, SHARE = F::SHARE;
    constexpr bool LATE = FT::LATE, early = FT::EARLY, FIN = FT::FIN, work2 = FT::WORK2;
    const int32_t l = active ? (int32_t)lb : 0;
    const int32_t i = ld.lo + l;

    // ---- K1 first: the contact search reads only step-start data -----------
    const Snap<T> self = xld(ld.snap_cur + i);
    const V3<T> x = {self.x, self.y, self.z};
    const int32_t ci = RB_ABLATE == 8 ? 0 : i;    // (diagnostic, load_body)
    // (LATE: the kind-dependent selects below wait for the search's overlap)
    int32_t kind = ld.cs.kind[ci];
    const T bi = self.r;
    // half extents y, z only matter for boxes; loaded for every body (a load
    // under a kind test would wait for kind before the state loads issue)
    T sy = ld.cs.sy()[ci], szz = ld.cs.sz()[ci];
    V3<T> sz = {ld.cs.sx()[ci], !LATE && kind != 0 ? sy : T(0), !LATE && kind != 0 ? szz : T(0)};
    [[maybe_unused]] auto late_kind = [&] {
        if constexpr (LATE) {
            asm volatile("" : "+v"(kind), "+v"(sy), "+v"(szz));
            sz.y = kind != 0 ? sy : T(0);
            sz.z = kind != 0 ? szz : T(0);
        }
    };
    BodyIn<T> in;
    LazyInvI<T> invI;
    bool forced = false;
    // (early: the state loads issued before the search)
    if constexpr (SHARE) {
        // both waves run this function (role 1: the helper wave, lane t for
        // the body of body lane t); the helper loads the state and constants
        if (role && active) {
            in = load_body(ld.st, ld.cs, l, i);
            invI.I = in.I;
            invI.q = in.q;
        }
    } else if constexpr (early && HELP && WIDE) {
        // the helper wave loads the state and constants (help_body) and hands
        // over q, m, inv(I_w) and the post-gravity, post-plane v and w: the
        // body lanes load only what the search needs (the cooperative form
        // keeps its own loads: handing q, m over there measured 4,096 bodies
        // 7.4 -> 7.9 us, 8,190 8.6 -> 9.0)
    } else if constexpr (early) {
        in = load_body(ld.st, ld.cs, l, i);
        invI.I = in.I;
        invI.q = in.q;
    }
    if constexpr (PRE) {
        // preloaded lead (step_body): the parameter block's fields the search
        // starts with — every one the bucket head addresses need — in one
        // scalar round trip under the body's loads (which needed none of
        // them).  One statement: each such statement waits for its operands
        if constexpr (EP) {
            // (the lead block's words too: the table's choice comes before
            // the head addresses; step_body issued their load first)
            asm volatile("" ::"s"(gen), "s"(ctrl), "s"(p.grid.inv_cs), "s"(p.grid.H), "s"(p.grid.super),
                         "s"(p.cur.line), "s"(p.n_global), "s"(p.xfrc), "s"(p.ep.line[0]), "s"(p.ep.line[1]),
                         "s"(p.ep.spill[0]), "s"(p.ep.spill[1]));
        } else {
            asm volatile("" ::"s"(p.grid.inv_cs), "s"(p.grid.H), "s"(p.grid.super), "s"(p.cur.line), "s"(p.cur.gen),
                         "s"(p.n_global), "s"(p.xfrc));
            if constexpr (G > 1) asm volatile("" ::"s"(p.cur.pos));
            // worlds without epochs need the generation only once the heads
            // are back: its load goes out here, ahead of theirs, and waits
            // with them.  (The scalar read of the lead block ahead of the
            // parameter block measured C2 6.98 -> 7.13 us per step in the
            // cooperative form: every scalar wait then also waits for it)
            gen = *p.cur.gen;
        }
    }
    // append epochs (EP: launches of worlds that run them, launch_step_wide;
    // rb_internal.hpp Epoch): the control word picks the table this step
    // reads and the one it inserts into
    Table<T> cur = p.cur, next = p.next;
    uint32_t gen_next = gen + 1u;
    bool ep_append = false;
    // the table can show appended entries (duplicates, stale ones): it has
    // been appended to by earlier steps, or this launch's own movers append
    // to it while other workgroups still read it.  Not in a rebuild step at
    // age 0: the step before built that table from every body, once each
    [[maybe_unused]] bool ep_appended = false;
    if constexpr (EP) {
        {
            const uint32_t cw = ctrl;                // (== *p.ep.ctrl: the lead block's word of this parity)
            const uint32_t t = cw & EP_TAB;
            ep_append = (cw & EP_APPEND) != 0;
            ep_appended = ep_append || ((cw >> EP_AGE_SHIFT) & 255u) != 0;
            const uint32_t tn = ep_append ? t : 1u - t;
            cur.line = t ? p.ep.line[1] : p.ep.line[0];
            cur.spill = t ? p.ep.spill[1] : p.ep.spill[0];
            next.line = tn ? p.ep.line[1] : p.ep.line[0];
            next.spill = tn ? p.ep.spill[1] : p.ep.spill[0];
            if (ep_append) gen_next = gen;
        }
    }
    [[maybe_unused]] uint32_t b0 = NO_BUCKET;    // the body's step-start bucket (wide search)
    STAMP(1);
    int32_t np_ = 0;
    bool defer = false;                          // a box-involved partner in range: the box kernel steps it
    [[maybe_unused]] int32_t n_half = 0;         // shared search: this wave's hits
    // what a helper wave has done for the body already (HelpDone)
    bool help_planes = false;
    int32_t help_nrec = 0;
    if constexpr (SHARE) {
        // the search shared between the two waves (rb_grid.hpp
        // search_half_wide): the body wave five of the eight buckets, the helper three.  The helper
        // does its work (help_body's: inv(I_w), gravity, plane contacts)
        // under its head loads, and, being the later of the two and the one
        // that holds the body's state in registers, finishes the body: the
        // body wave (role 0) only searches, leaves its hit count and defer
        // flag in s_half and is done at the one barrier
        M3<T> hm{};
        int32_t hrec = 0;
        bool hplanes = false;
        // gravity and the plane contacts (not with applied forces: body_update's)
        auto own_planes = [&] {
            if (p.xfrc) return;
            apply_force(p, l, in.m, invI, in.v, in.w);
            const T hk = impulse_k(in.m);
            if (kind == 0) solve_planes_sphere(p, p, l, x, sz.x, in.m, hk, invI, in.v, in.w, hrec);
            else solve_planes_box(p, p, l, x, mj_body_mat(in.q), sz, in.m, hk, invI, in.v, in.w, hrec);
            hplanes = true;
        };
        if (RB_ABLATE != 1 && active)
            n_half = search_half_wide<T, MAXP, EP>(
                p, i, x, role, s_id, s_cand, s_hpos, tid, gen, cur, b0,
                [&](uint32_t tj, const Snap<T> &s) { return candidate_hit<T, BOXES>(p, i, kind, x, sz.x, bi, tj, s, defer); },
                [&] {
                    if constexpr (LATE) late_kind();
                    if (!role) return;
                    hm = invI.get();
                    if (!work2) own_planes();
                },
                [&] {
                    if (!work2 || !role) return;
                    __builtin_amdgcn_sched_barrier(0);   // the candidate loads issue before the work
                    own_planes();
                });
        else if constexpr (LATE) late_kind();    // (no search: idle lanes, a diagnostic build)
        // the wave that does not finish leaves its hit count and defer flag
        if ((FIN ? !role : role) && active)
            s_half[tid] = (uint32_t)(n_half < 0xffff ? n_half : 0xffff) | (defer ? 1u << 16 : 0u);
#if RB_STAMPS
        if (role) STAMP(2);                      // the helper wave's last hit is written
#endif
        // every lane of both waves, idle ones too: the other wave's hits and
        // s_half are written, and both searches are done with s_cand (the
        // merge's scratch)
        __syncthreads();
        if constexpr (FIN) {
#if RB_STAMPS
            if (role) STAMP(11);                 // the finishing wave is past the barrier
            else STAMP(2);                       // the search-only wave's wait (10 -> 2) is over
#endif
            if (!role) return;
            if (active) defer |= (s_half[tid] >> 16) != 0;
            // inv(I_w), the post-gravity, post-plane v and w and the plane
            // contacts' record count, straight from this wave's registers (with
            // applied forces: body_update applies the force and solves the planes)
            invI.m = hm;
            invI.have = true;
            forced = hplanes;
            help_planes = hplanes;
            help_nrec = hrec;
        } else {
            // MAXP 32 instances: the helper hands its results over in the
            // list area, as help_body does, and the body wave finishes
            if (role && active) {
                T *o = s_help + tid;
#pragma unroll
                for (int e = 0; e < 9; ++e) o[(HELP_INVI + e) * NB] = hm.a[e];
                o[HELP_V * NB] = in.v.x; o[(HELP_V + 1) * NB] = in.v.y; o[(HELP_V + 2) * NB] = in.v.z;
                o[HELP_W * NB] = in.w.x; o[(HELP_W + 1) * NB] = in.w.y; o[(HELP_W + 2) * NB] = in.w.z;
                o[HELP_NREC * NB] = T(hplanes ? hrec : HELP_NO_PLANES);
                o[HELP_Q * NB] = in.q.w; o[(HELP_Q + 1) * NB] = in.q.x; o[(HELP_Q + 2) * NB] = in.q.y;
                o[(HELP_Q + 3) * NB] = in.q.z;
                o[HELP_M * NB] = in.m;
            }
            __syncthreads();
            if (role) return;
            if (active) defer |= (s_half[tid] >> 16) != 0;
#if RB_STAMPS
            STAMP(2);
#endif
        }
    } else if constexpr (G == 1 && WIDE && HELP) {
        // the helper wave evaluates inv(I_w), gravity and the plane contacts
        // (help_body); every lane of the body wave takes part in its two
        // barriers, so the search runs under the active mask only
        if (RB_ABLATE != 1 && active)
            np_ = search_partners_wide<T, MAXP, BOXES, EP>(p, i, kind, x, sz.x, bi, s_id, s_cand, s_didx, s_hpos, tid, gen,
                                                       cur, ep_appended, b0, defer, [] {});
        __syncthreads();                         // the search is done with s_cand: the helper fills it
        __syncthreads();
    } else if constexpr (G == 1 && WIDE) {
        if (RB_ABLATE != 1)
            np_ = search_partners_wide<T, MAXP, BOXES, EP>(p, i, kind, x, sz.x, bi, s_id, s_cand, s_didx, s_hpos, tid, gen,
                                                       cur, ep_appended, b0, defer, [&] {
                invI.get();
                if (!p.xfrc) {
                    apply_force(p, l, in.m, invI, in.v, in.w);
                    forced = true;
                }
            });
    } else if constexpr (G == 1) {
        if (RB_ABLATE != 1) np_ = search_partners<T, MAXP, BOXES>(p, i, kind, x, sz.x, bi, s_id, tid, gen, defer);
    } else if constexpr (HELP) {
        // the helper wave evaluates inv(I_w) and gravity (help_body)
        if (RB_ABLATE != 1)
            np_ = search_coop<T, MAXP, G, BOXES, 0>(p, active, i, kind, x, sz.x, bi, s_id, s_pos, t_id, t_pos, slot, k, tid,
                                                    gen, defer, [] {});
    } else {
        if (RB_ABLATE != 1)
            np_ = search_coop<T, MAXP, G, BOXES, 0>(p, active, i, kind, x, sz.x, bi, s_id, s_pos, t_id, t_pos, slot, k, tid,
                                          gen, defer, [&] {
                                              invI.get();
                                              if (!p.xfrc) {
                                                  apply_force(p, l, in.m, invI, in.v, in.w);
                                                  forced = true;
                                              }
                                          });
    }
    if constexpr (!SHARE) STAMP(2);              // (shared search: stamped at its barrier)
    if (RB_ABLATE == 7) np_ = 0;                 // diagnostic: search, but solve no partner contact
    if (!active || k != 0 || RB_ABLATE == 4) return;
    if (!BOXES && defer) {                       // box worlds only (p.defer_q set)
        // queued for the box kernel; chunks replayed without it (rb_api_step.hip
        // box_opt) only count, and are rolled back if the count is not zero
        const int32_t q = atomicAdd(p.defer_cnt, 1);
        if (q < p.S) p.defer_q[q] = l;
        return;
    }
    if constexpr (!early) {
        in = load_body(p, l, i);
        invI.I = in.I;
        invI.q = in.q;
    }
    if constexpr (HELP && !FIN) {
        // the helper's results (its LDS writes precede the search's barriers)
        const T *o = s_help + slot;
        constexpr int NBH = STEP_BLOCK / G;
#pragma unroll
        for (int e = 0; e < 9; ++e) invI.m.a[e] = o[(HELP_INVI + e) * NBH];
        invI.have = true;
        if (!p.xfrc) {
            in.v = {o[HELP_V * NBH], o[(HELP_V + 1) * NBH], o[(HELP_V + 2) * NBH]};
            in.w = {o[HELP_W * NBH], o[(HELP_W + 1) * NBH], o[(HELP_W + 2) * NBH]};
            forced = true;
        } else if constexpr (WIDE) {             // applied forces: the body lanes apply them
            in.v = {p.st.vx()[l], p.st.vy()[l], p.st.vz()[l]};
            in.w = {p.st.wx()[l], p.st.wy()[l], p.st.wz()[l]};
        }
        if constexpr (WIDE) {
            in.q = {o[HELP_Q * NBH], o[(HELP_Q + 1) * NBH], o[(HELP_Q + 2) * NBH], o[(HELP_Q + 3) * NBH]};
            in.m = o[HELP_M * NBH];
        }
        const T pr = o[HELP_NREC * NBH];
        help_planes = pr >= T(0);
        help_nrec = help_planes ? (int32_t)pr : 0;
    }
    // shared search: the two halves' hits, merged and ordered by the
    // finishing wave: the body wave's list (rows 0 up, its count from s_half)
    // and this wave's own (rows MAXP - 1 down)
    if constexpr (SHARE) {
        // the merge's scratch is the candidate list area this wave's search
        // read last: no access may move across this point
        asm volatile("" ::: "memory");
        if (RB_ABLATE != 1)
            np_ = FIN ? merge_halves<T, MAXP, EP>(p, s_id, s_cand, s_didx, tid, (int32_t)(s_half[tid] & 0xffffu), n_half, ep_appended)
                      : merge_halves<T, MAXP, EP>(p, s_id, s_cand, s_didx, tid, n_half, (int32_t)(s_half[tid] & 0xffffu), ep_appended);
        STAMP(7);
        if (RB_ABLATE == 7) np_ = 0;
    }
    constexpr int PM = FT::PM;
    body_update<T, typename FT::Update>(
        p, l, i, x, kind, sz, bi, in, forced, invI,
        Partners<T>{np_, s_id + slot, NB, PM == 2 ? s_hpos + slot : s_pos + slot, PM == 2 ? s_didx + slot : nullptr},
        HelpDone{help_nrec, help_planes}, NextTable<T>{gen_next, EP ? &next : nullptr, ep_append ? b0 : NO_BUCKET},
        tid, cell, BOXES ? s_poly + slot : nullptr, NB);
}

// Halo exchange: fold the wave's new cells, given as per-lane boxes
// (lo[0] == INT32_MAX: none), into the step's bound copies — one atomic
// min/max per axis per wave, on copy (block % BOUND_COPIES).  Every lane of
// the wave must call it.
__device__ __forceinline__ void fold_box(int32_t *bounds, int32_t lo[3], int32_t hi[3]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = min(lo[d], __shfl_xor(lo[d], off));
            hi[d] = max(hi[d], __shfl_xor(hi[d], off));
        }
    if ((threadIdx.x & 63) == 0 && lo[0] != INT32_MAX) {
        int32_t *c = bounds + (int64_t)(blockIdx.x % BOUND_COPIES) * BOUND_STRIDE;
#pragma unroll
        for (int d = 0; d < 3; ++d) { atomicMin(c + d, lo[d]); atomicMax(c + 3 + d, hi[d]); }
    }
}
// one cell per lane (cell[0] == INT32_MAX: none)
__device__ __forceinline__ void fold_bounds(int32_t *bounds, const int32_t *cell) {
    int32_t lo[3], hi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const bool have = cell[0] != INT32_MAX;
        lo[d] = have ? cell[d] : INT32_MAX;
        hi[d] = have ? cell[d] : INT32_MIN;
    }
    fold_box(bounds, lo, hi);
}

// Helper wave of the cooperative form (HELP): one lane per body of the
// workgroup evaluates inv(I_w), gravity and a sphere's plane contacts (the
// first in its contact order) — VALU chain the body lanes otherwise run
// under or after their bucket loads — and leaves inv(I_w), v, w and the
// recorded-contact count, q and m in LDS (the HELP_* rows, HELP_REALS per body) before
// the search's first barrier; it then takes part in the search's two
// barriers.  The same arithmetic in the same order, so bit-identical.
//
// WIDE (step_kernel_wide_help): the results go to the body wave's candidate
// list area once its search is done with it (between the two barriers),
// so the workgroup's LDS stays within a quarter of the CU's.
template <typename T, int NB, bool WIDE = false>
__device__ __forceinline__ void help_body(const StepParams<T> &p, const Lead<T> &ld, int h, T *s_help) {
    // the same block -> bodies mapping as the body lanes (step_body)
    const int64_t hb = (int64_t)xcd_block(blockIdx.x, gridDim.x) * NB + h;
    const bool act = h < NB && hb < ld.n_local;
    // results kept in registers across the wide form's first barrier; the
    // barriers themselves are outside every divergent branch (a barrier in
    // a branch taken by some lanes of the wave would be issued once per path)
    BodyIn<T> in{};
    M3<T> m{};
    int32_t nrec = 0;
    bool planes = false;
    if (act) {
        const int32_t l = (int32_t)hb, i = ld.lo + l;
        in = load_body(ld.st, ld.cs, l, i);
        LazyInvI<T> invI;
        invI.I = in.I;
        invI.q = in.q;
        m = invI.get();
        if (!p.xfrc) {
            apply_force(p, l, in.m, invI, in.v, in.w);
            // a body's plane contacts come first in its contact order
            // (rb_body.hpp), so they are solved here
            const int32_t kind = ld.cs.kind[i];
            const Snap<T> self = ld.snap_cur[i];
            const V3<T> x = {self.x, self.y, self.z};
            const T k = impulse_k(in.m);
            if (kind == 0) {
                solve_planes_sphere(p, p, l, x, ld.cs.sx()[i], in.m, k, invI, in.v, in.w, nrec);
            } else {
                const V3<T> sz = {ld.cs.sx()[i], ld.cs.sy()[i], ld.cs.sz()[i]};
                solve_planes_box(p, p, l, x, mj_body_mat(in.q), sz, in.m, k, invI, in.v, in.w, nrec);
            }
            planes = true;
        }
    }
    if (WIDE) __syncthreads();                   // the body wave's search is done with s_cand
    if (act) {
        T *o = s_help + h;
#pragma unroll
        for (int e = 0; e < 9; ++e) o[(HELP_INVI + e) * NB] = m.a[e];
        o[HELP_V * NB] = in.v.x; o[(HELP_V + 1) * NB] = in.v.y; o[(HELP_V + 2) * NB] = in.v.z;
        o[HELP_W * NB] = in.w.x; o[(HELP_W + 1) * NB] = in.w.y; o[(HELP_W + 2) * NB] = in.w.z;
        o[HELP_NREC * NB] = T(planes ? nrec : HELP_NO_PLANES);
        o[HELP_Q * NB] = in.q.w; o[(HELP_Q + 1) * NB] = in.q.x; o[(HELP_Q + 2) * NB] = in.q.y;
        o[(HELP_Q + 3) * NB] = in.q.z;
        o[HELP_M * NB] = in.m;
    }
    __syncthreads();
    if (!WIDE) __syncthreads();                  // search_coop's two barriers
}

// A step kernel of form F.  HALO: the halo push compiled in (checked at run
// time: p.halo.mail); the wide forms — the single-GPU bench's kernels — are
// also instantiated without it (launch_step_wide picks), which measured
// 1-2 % faster at C3.  Not a member of the form: body_step does not depend on
// it, and the kernels that differ only in it share one body_step.
template <typename T, typename F, bool HALO = true>
__device__ __forceinline__ void step_body(const StepParams<T> &p, const Lead<T> &ld) {
    constexpr int MAXP = F::MAXP, G = F::G, NB = FormTraits<F>::NB;
    constexpr bool WIDE = F::WIDE, BOXES = F::BOXES, HELP = F::HELP, EP = F::EP, SHARE = F::SHARE;
    static_assert(!EP || !HALO, "append epochs: never halo-exchanging");
    __shared__ int32_t s_id[MAXP * NB];
    __shared__ T s_poly[BOXES ? 48 * NB : 1];   // box-box face clipping: 2 x 8 vertices x 3 per body
    __shared__ uint32_t s_cand[WIDE ? WIDE_MAXC * NB : 1];
    __shared__ uint8_t s_didx[WIDE ? MAXP * NB : 1];
    __shared__ Snap<T> s_hpos[WIDE && RB_WIDE_LDSPOS ? WIDE_HPOS * NB : 1];
    __shared__ int32_t t_id[G > 1 ? MAXP * NB : 1];
    __shared__ Snap<T> s_pos[G > 1 ? MAXP * NB : 1];
    __shared__ Snap<T> t_pos[G > 1 ? MAXP * NB : 1];
    // the wide form's helper results share the candidate list's area
    __shared__ T s_help[HELP && !WIDE ? HELP_REALS * NB : 1];
    static_assert(!WIDE || sizeof(uint32_t) * WIDE_MAXC >= HELP_REALS * sizeof(T), "helper results fit in s_cand");
    T *const help_lds = WIDE ? reinterpret_cast<T *>(s_cand) : s_help;
    // shared search: the helper's hit count and defer flag, per body
    __shared__ uint32_t s_half[SHARE ? NB : 1];
    // (wave-uniform: the second wave of a SHARE workgroup runs body_step too)
    const int role = SHARE ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x / STEP_BLOCK)) : 0;
    const int tid = SHARE ? (int)(threadIdx.x % STEP_BLOCK) : (int)threadIdx.x;
    if (RB_ABLATE == 3) return;
    if constexpr (HELP && !SHARE) {
        if (tid >= STEP_BLOCK) {                 // the workgroup's second wave
            help_body<T, NB, WIDE>(p, ld, tid - STEP_BLOCK, help_lds);
            return;
        }
    }
    STAMP(0);
#if RB_STAMPS
    // placement: HW_ID (wave, SIMD, CU, SE fields) and XCC_ID of the block's first wave
    if (threadIdx.x == 0 && blockIdx.x < (1u << 16)) {
        rb_stamp_buf[blockIdx.x][15] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
        rb_stamp_buf[blockIdx.x][14] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
    }
#endif
    // worlds with append epochs: the kernel's first load is the lead block,
    // from preloaded SGPRs (after the first stamp of a diagnostic build,
    // which waits for scalar loads); the others: body_step
    LeadWords lw{0u, 0u};
    if constexpr (EP) {
        lw = lead_words(ld.gen_cur);
        __builtin_amdgcn_sched_barrier(0);
    }
    // The lead (the body's first loads' fields) is preloaded; body_step waits
    // for the parameter block's scalar loads only under the body's loads.
    // Block 0 advances the exchange's step number and publishes the next
    // table's generation (one more than the one this step reads) for the
    // kernels that insert after this one, at the end: a store ahead of the
    // body loads would hold them back (they may not pass it).

    const int slot = tid / G, k = tid % G;
    const int64_t lb = (int64_t)xcd_block(blockIdx.x, gridDim.x) * NB + slot;
    const int64_t halo_e = HALO && p.halo.mail ? *p.halo.halo_e : 0;   // (halo-exchanging shards: the push's epoch)
    const bool active = lb < ld.n_local;
    int32_t cell[6] = {INT32_MAX, 0, 0, 0, 0, 0};   // new cell, step-start cell (peer-to-peer exchange)
    if (G > 1 || HELP || active)                 // (a helper's barriers: every lane)
        body_step<T, F>(p, ld, active, lb, slot, k, tid, s_id, s_pos, t_id, t_pos,
                                                              s_cand, cell, lw.gen, s_poly, s_didx, s_hpos, help_lds, role,
                                                              s_half, lw.ctrl);
    // shared search: the body wave is done; the helper wave, which finished
    // the bodies, holds their cells and does the rest (its tid 0: block 0's stores)
    // (MAXP 32 instances: the body wave finishes and the helper is done)
    if (SHARE && (FormTraits<F>::FIN ? !role : role)) return;
    if (p.bounds) fold_bounds(p.bounds, cell);
    if (HALO && p.halo.mail) {                   // halo-exchanging shard: push to the peers
        int32_t b[6];
        if (halo_bounds(p, halo_e, b)) halo_push(p, halo_e, cell[0] != INT32_MAX, (int32_t)(ld.lo + lb), cell, b);
    }
    if (blockIdx.x == 0 && tid == 0) {
        bool same_gen = false;
        if constexpr (EP) {
            {
                // the next step's control word.  This step's appenders raise
                // crowd; the flag read here is the one of the step before
                // (complete), so the schedule is the same in every run.
                const uint32_t cw = *p.ep.ctrl;
                const uint32_t t = cw & EP_TAB, age = (cw >> EP_AGE_SHIFT) & 255u, len = (cw >> EP_LEN_SHIFT) & 255u;
                const uint32_t start = cw >> EP_START_SHIFT;
                const bool dirty = (cw & EP_DIRTY) || *p.ep.crowd_prev != 0;
                *p.ep.crowd_prev = 0;
                uint32_t nw;
                if (cw & EP_APPEND) {
                    // crowded: the next step rebuilds
                    nw = epoch_word(t, age + 1u, dirty ? age + 2u : len, dirty, start);
                    same_gen = true;
                    p.ep.count[0] += 1ull;
                } else {
                    // a clean epoch doubles the next one's length; a crowded one restarts at 1
                    // (short epochs while the scene starts up: rb_internal.hpp)
                    const uint32_t ns = min(start + 1u, 255u);
                    const uint32_t cap = ns < EP_START_REBUILDS ? min(EP_START_LEN, (uint32_t)p.ep.len_max) : (uint32_t)p.ep.len_max;
                    const uint32_t nl = dirty ? 1u : min(2u * len, cap);
                    nw = epoch_word(1u - t, 0u, nl, false, ns);
                    p.ep.count[1] += 1ull;
                }
                *p.ep.ctrl_next = nw;
            }
        }
        if (p.next.line) *p.next.gen = *p.cur.gen + (same_gen ? 0u : 1u);
        if (p.epoch) *p.epoch += 1;
    }
}

// The launchers' dispatch: pick(f, b...) calls f with each run-time choice b
// as a compile-time constant (std::true_type or std::false_type), so a
// launcher names a kernel family once and every instance of it is compiled.
// maxp_c: the partner bound of a "maxp <= 16" choice.
template <typename Fn> inline void pick(Fn f) { f(); }
template <typename Fn, typename... Bs> inline void pick(Fn f, bool b, Bs... bs) {
    if (b) pick([&](auto... c) { f(std::true_type{}, c...); }, bs...);
    else pick([&](auto... c) { f(std::false_type{}, c...); }, bs...);
}
constexpr int maxp_c(bool small) { return small ? 16 : 32; }

}  // namespace rb
