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

using namespace rb;

struct rb_world {
    int dtype = RB_F64, esz = 8, device = 0;
    hipStream_t stream = nullptr, own_stream = nullptr, cap_stream = nullptr;
    int64_t N = 0, S = 0, Npad = 0, lo = 0;
    int32_t n_local = 0, P = 1, rank = 0;
    int32_t n_planes = 0, oriented = 1, maxp = 16, maxrec = 0;
    // owned bodies up to which the cooperative search is used: above it
    // the wide form (with its helper wave) is faster (19,600: 14.4 vs 12.1
    // us; 16,384: 11.1 vs 11.3, 12,100: 10.4 vs 11.5 the other way;
    // profiles/r03/wide_help/ab_thresh_flat.txt)
    int64_t coop_max = 16384;
    // above coop_max, up to which the wide one-lane form is used; with its
    // helper wave it is at least as fast as the one-lane form at every size
    // measured (131k / 262k equal, 524k 0.116 -> 0.102 ms, 1M 0.236 ->
    // 0.216, 4M 0.876 -> 0.841; profiles/r03/wide_help/ab_large2.txt), so
    // the one-lane form only runs on request (RBHIP_WIDE_MAX_BODIES)
    int64_t wide_max = INT64_MAX;
    // owned bodies up to which the cooperative form runs with a helper wave
    // per workgroup (inv(I_w), gravity and plane contacts off the body
    // lanes' chain): 4k 8.1 -> 7.4 us, 8k 9.6 -> 8.6; 16k 11.0 -> 11.9 the
    // other way (its waves then share SIMDs)
    int64_t help_max = 12288;
    // the wide form with a helper wave per workgroup (inv(I_w), gravity,
    // plane contacts and the state / constant loads off the body wave;
    // A/B steps 261-460, profiles/r03/wide_help_ab.txt): 32k 13.6 -> 12.9
    // us, C3 16.8 -> 16.1, C4 15.4 -> 14.9, C5 (16,384 cubes) 12.1 -> 9.6
    bool wide_help = true;
    // that form with the contact search shared between its two waves: the
    // helper lane of a body searches four of its eight buckets (rb_grid.hpp
    // search_half_wide; RBHIP_HELP_SEARCH)
    bool help_search = true;
    double planes[RB_MAX_PLANES][6] = {};
    double g[3] = {};
    double inv_cs = 1.0;
    double rmax = 0.0;             // largest bounding radius
    bool all_spheres = true;
    bool boxes = false;            // box-capable step kernels (any box body; sharded worlds exchange orientations)
    // contact law (rb_set_contact_law)
    int32_t law = RB_LAW_MUJOCO;
    double tol = 0.01;
    double prm_dt = 0, prm_e = 0, prm_mu = 0;   // the ground phase held in the snapshots (two-ball law)
    int64_t H = 4096;
    int64_t hmax = 4096;           // the table's growth limit (RBHIP_HASH_MAX_BYTES)
    int32_t group = 0;             // Grid::super: bucket grouping shape (x | y << 4 | z << 8 bits)
    bool fit_valid = false;        // fit_period: the group box (and layout) the last fit was made for
    int64_t fit_key[7] = {};
    int64_t bytes_per_body_step = 0;
    std::vector<double> bound;     // host copy of every body's bounding radius (rb_set_state's snapshot rows)
    // device memory
    void *snap[2] = {};        // [Npad] Snap<T>: (x, y, z, bound radius), ping-pong
    void *qsnap[2] = {};       // boxes: [Npad][4] step-start orientations, ping-pong with snap
    int32_t *defer_q = nullptr;    // boxes: [S] bodies the step kernel defers to the box kernel
    int32_t *defer_cnt = nullptr;  // boxes: [2] queue lengths by step parity
    // box worlds, one rank: chunks of steps replay optimistically WITHOUT the
    // box kernel (an idle one still costs a kernel boundary per step); the
    // step kernels then only count deferrals, and a chunk that deferred any
    // body is rolled back to its start and replayed with the box kernel
    bool box_opt = true;           // RBHIP_BOX_OPTIMISTIC=0: always launch the box kernel
    bool box_kernel_on = true;     // launch_one: the box kernel follows the step kernel
    int32_t box_backoff = 0;       // chunks to run with the box kernel after a rollback (doubles)
    int32_t box_skip = 0;          // of which left
    void *opt_save = nullptr;      // chunk-start copy: state rows, snapshot, orientations, error word
    int32_t *defer_host = nullptr; // pinned [2]
    int64_t box_stats[2] = {};     // optimistic chunks, rollbacks
    bool sync_call = false;        // inside rb_step (synchronous): long chunks are guarded
    int64_t refits = 0;            // layout refits after a bucket overflow (rolled back, replayed)
    int64_t table_grows = 0;       // of which with the table doubled
    int64_t partner_grows = 0;     // max_partners raised 16 -> 32 after a partner overflow
    int32_t diag_overflow = 0;     // RBHIP_DIAG_OVERFLOW=n (tests): the next n guarded chunk checks
                                   // report a bucket overflow (the roll-back / refit / growth path)
    void *state = nullptr;     // 13 x S  (qw qx qy qz vx vy vz wx wy wz px py pz)
    void *vel[2] = {};         // two-ball law: [Npad] Vel<T>, ping-pong with the snapshots
    void *consts = nullptr;    // 8 x Npad (mass ix iy iz sx sy sz bound)
    int32_t *kind = nullptr;   // Npad
    void *xfrc = nullptr;      // 6 x S or null
    uint32_t *ids[2] = {};     // [H][LINE_WORDS] bucket blocks (rb_internal.hpp Table; alternate with the snapshots)
    uint32_t *spill[2] = {};   // [SPILL_LINES x SPILL_LINE_WORDS] ids past full buckets, per table
    void *pos[2] = {};         // [H][LINE_WORDS] Snap<T> bucket slot snapshots
    // the step kernels' lead block (rb_internal.hpp LEAD_WORDS), one allocation:
    // generations [2] and epoch control words [2] by step parity.  prime()
    // writes the current parity's words; the step kernels' block 0 the other's
    uint32_t *lead_blk = nullptr;
    uint32_t *gen = nullptr;   // [2] generation of the table of each step parity (rb_internal.hpp Table): lead_blk + LEAD_GEN
    uint32_t gen_off = 1;      // an upper bound of step c's generation: gen_off + c (host bookkeeping; only
                               // grows; append steps keep their table's generation, so the device's lag it)
    // append epochs (rb_internal.hpp Epoch): the control words [2] by step
    // parity are lead_blk + LEAD_CTRL; ep_mem, one allocation — two unused
    // words, crowding flags [2], counters [2] (append steps, rebuild steps)
    int32_t epoch_max = EPOCH_DEFAULT;   // RBHIP_TABLE_EPOCH; 1: every step rebuilds its next table
    uint32_t *ep_mem = nullptr;
    uint32_t *ep_ctrl() const { return lead_blk + LEAD_CTRL; }
    bool ep_primed = false;        // the last prime() started an epoch schedule
    int32_t *plist = nullptr;      // split form: [MAXP][S] sorted partner ids
    int32_t *plist_cnt = nullptr;  // split form: [S] partner counts
    int32_t *err = nullptr;
    int32_t *err_host = nullptr;   // pinned, device-mapped (publish_err_kernel writes it)
    int32_t *err_host_d = nullptr;
    // err_host holds the error word as of all error-writing work enqueued so
    // far: set by a graph launch (every captured graph ends in
    // publish_err_kernel), cleared by every builder of kernel parameters that
    // carry the error word and by every write to it.  rb_sync / rb_step then
    // only synchronise the stream.
    bool err_pub = false;
    ncclComm_t comm = nullptr;     // rb_shard_comm_init: the in-library exchange
    // peer-to-peer exchange (rb_p2p_connect)
    bool p2p = false;
    int64_t *flags = nullptr;      // the mailbox (MailLayout, uncached); starts with flags[P]: peer q
                                   // writes slot q when its step is done
    bool halo = false;             // rb_p2p_halo: push only the bodies a peer can reach
    int32_t *bounds = nullptr;     // peer-to-peer: [2][BOUND_COPIES][BOUND_STRIDE] own cell bounds (step parity)
    int32_t *push_cnt = nullptr;   // halo: [P] bodies pushed to each peer this step
    int64_t *halo_e = nullptr;     // halo: the epoch the next step kernel's pushes test against
    int64_t *epoch = nullptr;      // steps taken since connect (advanced by the step kernel)
    void **peer_snap_dev = nullptr;       // [2][P] device array: each rank's snapshot buffers
    void **peer_quat_dev = nullptr;       // box worlds: [2][P] each rank's orientation snapshots
    int64_t **peer_flags_dev = nullptr;   // [P] device array: each rank's flag array
    std::vector<void *> ipc_opened;       // peer mappings to close
    // recording
    bool record = false;
    int32_t *rec_count = nullptr, *rec_partner = nullptr, *rec_kind = nullptr;
    void *rec_dist = nullptr;
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
    double *io_q_h = nullptr, *io_v_h = nullptr;   // pinned [N][7], [N][6]
    double *io_q_hd = nullptr, *io_v_hd = nullptr; // the same pinned rows, device-mapped (rb_get_state's kernel writes them)
    hipEvent_t io_ev[4] = {};      // rb_get_state (RBHIP_IO_OUT=1): the download in chunks, each copied out as it lands
    double *io_q_d = nullptr, *io_v_d = nullptr;   // device
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
    int tile_mode = -1;            // RBHIP_TILE: 0 off, 1 every eligible world, -1 auto (default: >= tile_min_bodies, off after a roll-back)
    int tile_mode_init = -1;       // the mode at creation (auto: re-armed by an rb_set_state that uploads)
    int32_t tile_ntypes = 0;       // distinct (m, I) of the bodies when <= TILE_TYPES (else 0: no tile form)
    double tile_type_val[TILE_TYPES][4] = {};   // m ix iy iz of each type
    uint8_t *tile_type_of = nullptr;   // [N]
    int64_t tile_min_bodies = 65537;    // (the hashed forms win up to C3's 65,536 bodies, the tile form above: DESIGN §4.1)
    int32_t tile_tc = 0, tile_ntx = 0, tile_nty = 0, tile_cap = TILE_THREADS;
    bool tile_fit_valid = false;
    int tile_valid_sp = -1;        // the bins of this parity hold the state at step c (-1: no bins)
    void *tile_mem = nullptr;      // bins x 2 (column tables, positions, ids, state), far lists x 2
    size_t tile_mem_bytes = 0;
    int32_t *tile_fill = nullptr;  // build scratch [slots][TILE_OFFW]
    uint32_t *tile_gen = nullptr;  // [2] generation of each parity's bins (far-list tags)
    int32_t *tile_why = nullptr;   // TILE_WHY_* bits raised (device)
    unsigned long long *tile_commits = nullptr;   // runs committed by the unbin kernel (device)
    int64_t *tile_host = nullptr;  // pinned: err, why, commits
    int64_t *tile_pub_host = nullptr, *tile_pub_host_d = nullptr;   // pinned, mapped: why, commits (tile graphs' publish)
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
    uint32_t *cq_line = nullptr, *cq_spill = nullptr, *cq_words = nullptr;
    int64_t cq_H = 0;
    int32_t cq_layout = 0;
    uint32_t cq_gen = 0;           // the generation of the last query (0: the table holds zeros)
    char *cq_stage = nullptr, *cq_stage_h = nullptr;
    size_t cq_stage_bytes = 0;
    size_t cq_limit = (size_t)256 << 20;   // RBHIP_CONTACT_STAGE_BYTES

    int sp() const { return (int)(c % 2); }
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

// A device buffer that only grows: afterwards *buf holds `need` bytes or more.
// (The capacity is zero while the buffer is being replaced: an error in between
// leaves an empty buffer, not a dangling one.)
int grow(void **buf, size_t *cap, size_t need);
// Every array of a device form that is given: device memory on `device`.
// owner: "batch" / "world", for the message.  (A refusal leaves no HIP error behind.)
int dev_ptrs(int device, const char *owner, std::initializer_list<std::pair<const void *, const char *>> arrays);
// the bodies of a host-form query whose true count is past R
inline int64_t count_truncated(const int32_t *counts, size_t bodies, int32_t R) {
    int64_t t = 0;
    for (size_t k = 0; k < bodies; ++k) t += counts[k] > R;
    return t;
}

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
int snapshot_to_host(rb_world *w, std::vector<double> &rows);
int refit_from_device(rb_world *w, bool force = true);
int enqueue_steps(rb_world *w, int64_t nsteps, double dt, double e, double mu, double thr, bool sharded = false);

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
