// rb_host.hpp — what the host units of the C-ABI implementation (rb_api_*.hip)
// share: the world, the error plumbing, the thread gate's scopes, the dtype
// dispatch and the functions that cross units.  Not part of the public
// interface.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types only: RCCL is dlopen'ed by the sharded path

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <initializer_list>
#include <map>
#include <tuple>
#include <vector>

#include "../../include/rbhip.h"
#include "rb_internal.hpp"
#include "rb_owned.hpp"
#include "rb_worldplan.hpp"

using namespace rb;
using rb::host::DevBuf;
using rb::host::HostBuf;

// A world starts as its plan (rb_worldplan.hpp WorldPlan: the shard, the form
// thresholds, the table and its layout word, the switches).  Growth and refits
// move maxp, maxrec, H and group; the tile form's retirement, tile_mode
struct rb_world : WorldPlan {
    int dtype = RB_F64, esz = 8, device = 0;
    hipStream_t stream = nullptr, own_stream = nullptr, cap_stream = nullptr;
    int64_t N = 0;
    int32_t P = 1, rank = 0;
    int32_t n_planes = 0, oriented = 1;
    double planes[RB_MAX_PLANES][6] = {};
    double g[3] = {};
    double inv_cs = 1.0;
    double rmax = 0.0;             // largest bounding radius
    bool all_spheres = true;
    // contact law (rb_set_contact_law)
    int32_t law = RB_LAW_MUJOCO;
    double tol = 0.01;
    double prm_dt = 0, prm_e = 0, prm_mu = 0;   // the ground phase held in the snapshots (two-ball law)
    bool fit_valid = false;        // fit_period: the group box (and layout) the last fit was made for
    int64_t fit_key[7] = {};
    std::vector<double> bound;     // host copy of every body's bounding radius (rb_set_state's snapshot rows)
    // device memory (rb_owned.hpp: every buffer below is released with the world)
    DevBuf<void> snap[2];       // [Npad] Snap<T>: (x, y, z, bound radius), ping-pong
    DevBuf<void> qsnap[2];      // boxes: [Npad][4] step-start orientations, ping-pong with snap
    DevBuf<int32_t> defer_q;      // boxes: [S] bodies the step kernel defers to the box kernel
    DevBuf<int32_t> defer_cnt;    // boxes: [2] queue lengths by step parity
    // box worlds, one rank: chunks of steps replay optimistically WITHOUT the
    // box kernel (an idle one still costs a kernel boundary per step); the
    // step kernels then only count deferrals, and a chunk that deferred any
    // body is rolled back to its start and replayed with the box kernel
    // (if box_opt, the plan's)
    bool box_kernel_on = true;     // launch_one: the box kernel follows the step kernel
    int32_t box_backoff = 0;       // chunks to run with the box kernel after a rollback (doubles)
    int32_t box_skip = 0;          // of which left
    DevBuf<void> opt_save;        // chunk-start copy: state rows, snapshot, orientations, error word
    HostBuf<int32_t> defer_host;   // pinned [2]
    int64_t box_stats[2] = {};     // optimistic chunks, rollbacks
    bool sync_call = false;        // inside rb_step (synchronous): long chunks are guarded
    int64_t refits = 0;            // layout refits after a bucket overflow (rolled back, replayed)
    int64_t table_grows = 0;       // of which with the table doubled
    int64_t partner_grows = 0;     // max_partners raised 16 -> 32 after a partner overflow
    DevBuf<void> state;       // 13 x S  (qw qx qy qz vx vy vz wx wy wz px py pz)
    DevBuf<void> vel[2];        // two-ball law: [Npad] Vel<T>, ping-pong with the snapshots
    DevBuf<void> consts;      // 8 x Npad (mass ix iy iz sx sy sz bound)
    DevBuf<int32_t> kind;     // Npad
    DevBuf<void> xfrc;        // 6 x S or null
    DevBuf<uint32_t> ids[2];    // [H][LINE_WORDS] bucket blocks (rb_internal.hpp Table; alternate with the snapshots)
    DevBuf<uint32_t> spill[2];  // [SPILL_LINES x SPILL_LINE_WORDS] ids past full buckets, per table
    DevBuf<void> pos[2];        // [H][LINE_WORDS] Snap<T> bucket slot snapshots
    // the step kernels' lead block (rb_internal.hpp LEAD_WORDS), one allocation:
    // generations [2] and epoch control words [2] by step parity.  prime()
    // writes the current parity's words; the step kernels' block 0 the other's
    DevBuf<uint32_t> lead_blk;
    uint32_t *gen = nullptr;   // [2] generation of the table of each step parity (rb_internal.hpp Table): lead_blk + LEAD_GEN
    uint32_t gen_off = 1;      // an upper bound of step c's generation: gen_off + c (host bookkeeping; only
                               // grows; append steps keep their table's generation, so the device's lag it)
    // append epochs (rb_internal.hpp Epoch): the control words [2] by step
    // parity are lead_blk + LEAD_CTRL; ep_mem, one allocation — two unused
    // words, crowding flags [2], counters [2] (append steps, rebuild steps)
    DevBuf<uint32_t> ep_mem;
    uint32_t *ep_ctrl() const { return lead_blk + LEAD_CTRL; }
    bool ep_primed = false;        // the last prime() started an epoch schedule
    DevBuf<int32_t> plist;        // split form: [MAXP][S] sorted partner ids
    DevBuf<int32_t> plist_cnt;    // split form: [S] partner counts
    DevBuf<int32_t> err;
    HostBuf<int32_t> err_host;     // pinned, device-mapped (publish_err_kernel writes it)
    // err_host holds the error word as of all error-writing work enqueued so
    // far: set by a graph launch (every captured graph ends in
    // publish_err_kernel), cleared by every builder of kernel parameters that
    // carry the error word and by every write to it.  rb_sync / rb_step then
    // only synchronise the stream.
    bool err_pub = false;
    ncclComm_t comm = nullptr;     // rb_shard_comm_init: the in-library exchange
    // peer-to-peer exchange (rb_p2p_connect)
    bool p2p = false;
    DevBuf<int64_t> flags;        // the mailbox (MailLayout, uncached); starts with flags[P]: peer q
                                   // writes slot q when its step is done
    bool halo = false;             // rb_p2p_halo: push only the bodies a peer can reach
    DevBuf<int32_t> bounds;       // peer-to-peer: [2][BOUND_COPIES][BOUND_STRIDE] own cell bounds (step parity)
    DevBuf<int32_t> push_cnt;     // halo: [P] bodies pushed to each peer this step
    DevBuf<int64_t> halo_e;       // halo: the epoch the next step kernel's pushes test against
    DevBuf<int64_t> epoch;        // steps taken since connect (advanced by the step kernel)
    DevBuf<void *> peer_snap_dev;        // [2][P] device array: each rank's snapshot buffers
    DevBuf<void *> peer_quat_dev;        // box worlds: [2][P] each rank's orientation snapshots
    DevBuf<int64_t *> peer_flags_dev;  // [P] device array: each rank's flag array
    std::vector<void *> ipc_opened;       // peer mappings to close
    // recording
    bool record = false;
    DevBuf<int32_t> rec_count, rec_partner, rec_kind;
    DevBuf<void> rec_dist;
    // stepping state: step counter c; bucket counts rotate mod 3, snapshots
    // and bucket slots mod 2
    int64_t c = 0;
    bool primed = false;
    // captured K-step graphs, least recently used evicted past GRAPH_CACHE_MAX
    // entries (a caller stepping varying chunk lengths would otherwise keep
    // accumulating executables)
    struct GraphEntry { hipGraphExec_t ex; uint64_t used; };
    std::map<std::tuple<int64_t, int, double, double, double, double, int>, GraphEntry> graphs;
    uint64_t graph_tick = 0;
    // the boundary's staging (rb_set_state / rb_get_state): pinned host rows
    // in the caller's layout and their device twins, moved with one DMA each
    // way and transposed by a kernel.  The staging mirrors the device state
    // while mirror_version == state_version (every change of the state bumps
    // it): an rb_set_state with exactly those bytes is then a no-op
    HostBuf<double> io_q_h, io_v_h;                // pinned [N][7], [N][6], device-mapped (rb_get_state's kernel writes them)
    hipEvent_t io_ev[4] = {};      // rb_get_state (RBHIP_IO_OUT=1): the download in chunks, each copied out as it lands
    DevBuf<double> io_q_d, io_v_d;                 // device
    int64_t state_version = 0, mirror_version = -1;
    int64_t io_stats[2] = {};      // rb_set_state calls skipped (unchanged), uploads
    // kernel timing
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tev;
    double t_sum_ms = 0;
    int64_t t_n = 0;

    // cell-ordered tile form (rb_tiles.hip): sphere worlds on
    // one rank step in tile slots when eligible (tile_eligible).  The bins
    // (the state sorted by column, per step parity) are a cache of the
    // id-ordered state rows and snapshot: built from them at the first tile
    // run, carried from run to run, written back at the end of each run by
    // the unbin kernel — only if no step of it raised ERR_TILE, so that a
    // failed run leaves the id-ordered state at the start of the first
    // failed run, which the host replays with the hashed-cell forms
    // (tile_finish) at the next sync point.
    int tile_mode_init = -1;       // the mode at creation (auto: re-armed by an rb_set_state that uploads)
    int32_t tile_ntypes = 0;       // distinct (m, I) of the bodies when <= TILE_TYPES (else 0: no tile form)
    double tile_type_val[TILE_TYPES][4] = {};   // m ix iy iz of each type
    DevBuf<uint8_t> tile_type_of;     // [N]
    int32_t tile_tc = 0, tile_ntx = 0, tile_nty = 0, tile_cap = TILE_THREADS;
    bool tile_fit_valid = false;
    int tile_valid_sp = -1;        // the bins of this parity hold the state at step c (-1: no bins)
    DevBuf<void> tile_mem;         // bins x 2 (column tables, positions, ids, state), far lists x 2
    DevBuf<int32_t> tile_fill;    // build scratch [slots][TILE_OFFW]
    DevBuf<uint32_t> tile_gen;    // [2] generation of each parity's bins (far-list tags)
    DevBuf<int32_t> tile_why;     // TILE_WHY_* bits raised (device)
    DevBuf<unsigned long long> tile_commits;  // runs committed by the unbin kernel (device)
    HostBuf<int64_t> tile_host;   // pinned: err, why, commits
    HostBuf<int64_t> tile_pub_host;                               // pinned, mapped: why, commits (tile graphs' publish)
    bool tile_pub = false;         // err_pub, and the last graph was a tile run's (tile_pub_host is current)
    unsigned long long tile_commits_seen = 0;
    // a tile run whose check waits for the next sync point
    struct TileRun { int64_t c0, n; double dt, e, mu, thr; };
    std::vector<TileRun> tile_pending;    // runs enqueued since the last check
    int64_t tile_stats[4] = {};    // runs, steps committed, runs rolled back, bin builds
    int32_t tile_why_seen = 0;     // why bits of the runs rolled back (OR)
    int32_t tile_backoff = 0, tile_skip = 0;   // eligible runs to step hashed after a roll-back (doubling)
    bool tile_replaying = false;   // tile_finish's replay steps hashed

    // the contact query (rb_api_contacts.hip): a broadphase table of its own
    // (allocated at the first query; cq_words: its generation and its error
    // word) for the grid of cq_H buckets and line layout cq_layout, and the
    // host form's staging (device, pinned twin; at most cq_limit bytes).
    // Nothing else of the world is written by a query
    DevBuf<uint32_t> cq_line, cq_spill, cq_words;
    int64_t cq_H = 0;
    int32_t cq_layout = 0;
    uint32_t cq_gen = 0;           // the generation of the last query (0: the table holds zeros)
    DevBuf<char> cq_stage;
    HostBuf<char> cq_stage_h;
    size_t cq_stage_bytes = 0;

    int sp() const { return (int)(c % 2); }
    __attribute__((visibility("hidden"))) ~rb_world() = default;   // (the owners release the buffers: free_world)
};

// Everything the host units share beyond the world lives in rb::host, hidden:
// only the extern "C" rb_* entries join the library's dynamic symbols.
namespace rb {
namespace host __attribute__((visibility("hidden"))) {

// ---- rb_api_common.hip: errors and the thread gate --------------------------
// sets the calling thread's rb_last_error text; returns code
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// the device error word's bits as an error code (and text)
int err_to_code(int32_t bits);

// Every entry point runs inside an ApiScope of its world's device (-1: no
// device, or no valid world), a graph capture inside a CaptureScope.
struct ApiScope {
    explicit ApiScope(int device);
    ~ApiScope();
    ApiScope(const ApiScope &) = delete;
    ApiScope &operator=(const ApiScope &) = delete;
};
struct CaptureScope {   // (inside an ApiScope of a device: the capture's)
    int d;
    CaptureScope();
    ~CaptureScope();
    CaptureScope(const CaptureScope &) = delete;
    CaptureScope &operator=(const CaptureScope &) = delete;
};

#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(e_ == hipErrorOutOfMemory ? RB_ENOMEM : RB_ENODEV, "%s: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                           \
    } while (0)

// Every fill and copy of a world's buffers is enqueued on the world's own
// stream (w->stream), so it is ordered with the world's kernels by
// construction: a null-stream hipMemset / hipMemcpy is not ordered with a
// non-blocking stream (one once zeroed contact counts a step had just
// recorded), and a null-stream call also invalidates another thread's
// graph capture on the device.  Copies from or into host memory the caller
// frees on return end with a sync of that stream.
#define WCHK(expr)                                                                            \
    do {                                                                                      \
        if (int rc_ = (expr)) return rc_;                                                     \
    } while (0)

// stream-ordered fills and copies of world buffers (WCHK above)
inline int wfill(rb_world *w, void *dst, int value, size_t bytes) {
    HIPCHK(hipMemsetAsync(dst, value, bytes, w->stream));
    return RB_OK;
}
// from host memory the caller may free on return: waits for the copy
inline int wput(rb_world *w, void *dst, const void *src, size_t bytes) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    return RB_OK;
}
// into host memory: ordered after the world's work so far, waited for
inline int wget(rb_world *w, void *dst, const void *src, size_t bytes) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    return RB_OK;
}

// Every array of a device form that is given: device memory on `device`.
// owner: "batch" / "world", for the message.  (A refusal leaves no HIP error behind.)
int dev_ptrs(int device, const char *owner, std::initializer_list<std::pair<const void *, const char *>> arrays);
// the bodies of a host-form query whose true count is past R
inline int64_t count_truncated(const int32_t *counts, size_t bodies, int32_t R) {
    int64_t t = 0;
    for (size_t k = 0; k < bodies; ++k) t += counts[k] > R;
    return t;
}

// the byte counts of this world's buffers (rb_worldplan.hpp)
inline size_t snap_bytes(const rb_world *w) { return rb::snap_bytes(w->esz, w->Npad); }
inline size_t state_bytes(const rb_world *w) { return rb::state_bytes(w->esz, w->S); }
inline size_t consts_bytes(const rb_world *w) { return rb::consts_bytes(w->esz, w->Npad); }
inline size_t slot_snapshot_bytes(const rb_world *w) { return rb::slot_snapshot_bytes(w->esz, w->H); }
inline size_t record_slots(const rb_world *w) { return rb::record_slots(w->maxrec, w->S); }

template <typename T> T *dp(void *p, int64_t off) { return reinterpret_cast<T *>(p) + off; }

// f(T{}) with T the real type of dtype: by_real(w->dtype, [&](auto t) { using T = decltype(t); ... })
template <typename F> auto by_real(int dtype, F &&f) { return dtype == RB_F64 ? f(double{}) : f(float{}); }

// ---- rb_api_step.hip ---------------------------------------------------------
int step_form(const rb_world *w);
bool epoch_eligible(const rb_world *w);
template <typename T>
StepParams<T> make_step(rb_world *w, int64_t c, double dt, double e, double mu, double thr, bool insert_next);
template <typename T>
InsertParams<T> make_insert(rb_world *w, int sp, int64_t first, int64_t count, int64_t skip_lo, int64_t skip_hi);
int prime(rb_world *w, double dt = 0, double e = 0, double mu = 0);
int launch_one(rb_world *w, hipStream_t s, int64_t c, double dt, double e, double mu, double thr);
int timed_launch(rb_world *w, double dt, double e, double mu, double thr);
int collect_timing(rb_world *w);
void drop_graphs(rb_world *w);
int graph_replay(rb_world *w, int64_t K, int variant, double dt, double e, double mu, double thr,
                 const std::function<int(hipStream_t, int64_t)> &seq);
int gen_guard(rb_world *w, int64_t nsteps);
int enqueue_steps(rb_world *w, int64_t nsteps, double dt, double e, double mu, double thr, bool sharded = false);

// ---- rb_api_guard.hip --------------------------------------------------------
constexpr int64_t GUARD_MIN_STEPS = 64;   // shorter synchronous calls are not guarded (their
                                          // save + check would cost a few % of the call)
int guarded_chunk(rb_world *w, int64_t &K, int64_t left, bool opt, double dt, double e, double mu,
                  const std::function<int(int64_t, bool)> &replay);
int snapshot_to_host(rb_world *w, std::vector<double> &rows);
int refit_from_device(rb_world *w, bool force = true);

// ---- rb_api_tiles.hip --------------------------------------------------------
constexpr int TILE_DECLINED = 1;   // tile_run: the auto mode gave the form up; the world steps hashed
bool tile_eligible(const rb_world *w);
int tile_run(rb_world *w, int64_t n, double dt, double e, double mu, double thr);
int tile_finish(rb_world *w);
// every run that awaits its check at the next sync point (tile runs)
inline int finish_pending(rb_world *w) { return tile_finish(w); }

// ---- rb_api_shard.hip --------------------------------------------------------
int halo_prime(rb_world *w);
int shard_exchange(rb_world *w, hipStream_t s, int64_t c);
int shard_one(rb_world *w, hipStream_t s, int64_t c, double dt, double e, double mu, double thr);
void shard_release(rb_world *w);

// ---- rb_api_state.hip --------------------------------------------------------
void fit_period(rb_world *w, const double *qpos, bool force = false);

}  // namespace host
}  // namespace rb
