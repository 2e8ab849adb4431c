// rb_api_state.hip — the boundary: rb_set_state / rb_get_state with their
// pinned staging, and the fit of the table layout's period to the state.
#include "rb_host.hpp"
#include "rb_hostpool.hpp"
#include "rb_period.hpp"

namespace rb::host {

static int io_alloc(rb_world *w) {
    if (w->io_q_h) return RB_OK;
    const size_t nq = (size_t)7 * w->N, nv = (size_t)6 * w->N;
    // mapped and coherent: rb_get_state's kernel stores into them across
    // PCIe, visible to the host once the stream is synchronised
    WCHK(w->io_q_h.alloc(sizeof(double) * nq, hipHostMallocMapped | hipHostMallocCoherent));
    WCHK(w->io_v_h.alloc(sizeof(double) * nv, hipHostMallocMapped | hipHostMallocCoherent));
    WCHK(w->io_q_d.alloc(sizeof(double) * nq));
    WCHK(w->io_v_d.alloc(sizeof(double) * nv));
    return RB_OK;
}

template <typename T> static StateIO<T> make_io(rb_world *w) {
    StateIO<T> p{};
    p.qpos = w->io_q_d;
    p.qvel = w->io_v_d;
    p.snap = dp<Snap<T>>(w->snap[w->sp()], 0);
    p.quat = w->boxes ? dp<T>(w->qsnap[w->sp()], 0) : nullptr;
    p.st = BodyState<T>{dp<T>(w->state, 0), w->S};
    p.bound = dp<T>(w->consts, 7 * w->Npad);
    p.N = w->N;
    p.lo = w->lo;
    p.n_local = w->n_local;
    p.balls = w->law == RB_LAW_BALLS;
    return p;
}

// The linear cell layout's period (rb_grid.hpp bucket_linear): how the
// table's group bits split over x, y, z.  A split folds the scene onto
// itself where two groups a search reads (the occupied groups and their
// neighbours) land on one run of buckets with at least one of them occupied:
// those buckets then hold bodies of both, i.e. false candidates.  Every
// split is scored by that count of colliding groups and the least is taken;
// ties go to the split that leaves the fewest axes folded (a sheet folded
// along one axis stays collision-free as it moves; folded along two, only
// while the fold happens to miss it), then to the one whose period covers
// the scene's extent most evenly.
// Splitting by extent alone (one bit at a time to the axis the period covers
// least) folded a sheet-like scene — C4's spheres on the incline, whose
// bounding box is deep in z but whose groups are one layer thick — in x and
// y to cover z: 14.8 -> 18.1 us per step; counting collisions keeps C4's
// layout and still fits 4M flat spheres (1.33 -> 0.87 ms) and 32k on a
// 128 x 256 grid (17.9 -> 13.2 us).  Deterministic in the global positions,
// so every rank of a sharded world picks the same split.
void fit_period(rb_world *w, const double *qpos, bool force) {
    if (!layout_linear(w->group)) return;                 // hashed layouts have no period
    if (const char *ev = getenv("RBHIP_FIT_PERIOD"))
        if (atoi(ev) == 0) return;                       // diagnostic: keep the creation-time split
    const int gb[3] = {shape_bits(w->group, 0), shape_bits(w->group, 1), shape_bits(w->group, 2)};
    const int lg = period_bits(w->group);
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    std::vector<int64_t> occ;
    occ.reserve((size_t)w->N);
    for (int64_t b = 0; b < w->N; ++b) {
        int64_t g[3];
        bool ok = true;
        for (int d = 0; d < 3; ++d) {
            const double c = qpos[7 * b + d] * w->inv_cs;
            if (!(c == c && c > -1e9 && c < 1e9)) { ok = false; break; }
            lo[d] = c < lo[d] ? c : lo[d];
            hi[d] = c > hi[d] ? c : hi[d];
            g[d] = (int64_t)floor(c) >> gb[d];
            if (g[d] <= -PERIOD_OFF + 1 || g[d] >= PERIOD_OFF - 1) ok = false;
        }
        if (ok) occ.push_back(period_pack(g[0], g[1], g[2]));
    }
    // the split depends on the occupied groups; a call whose groups span
    // the same box as the last fit's (every frame of a per-frame caller:
    // multi_sphere_bounce.py:42 runs once per frame) keeps that fit instead
    // of re-sorting every split (RBHIP_FIT_PERIOD=2 always refits)
    {
        int64_t gb_lo[3] = {INT64_MAX, INT64_MAX, INT64_MAX}, gb_hi[3] = {INT64_MIN, INT64_MIN, INT64_MIN};
        for (int64_t k : occ)
            for (int d = 0; d < 3; ++d) {
                gb_lo[d] = std::min(gb_lo[d], period_unpack(k, d));
                gb_hi[d] = std::max(gb_hi[d], period_unpack(k, d));
            }
        const int64_t key[7] = {gb_lo[0], gb_lo[1], gb_lo[2], gb_hi[0], gb_hi[1], gb_hi[2], (int64_t)w->group};
        const char *ev = getenv("RBHIP_FIT_PERIOD");
        if (!force && w->fit_valid && memcmp(key, w->fit_key, sizeof key) == 0 && !(ev && atoi(ev) == 2)) return;
        memcpy(w->fit_key, key, sizeof key);
        w->fit_valid = true;
    }
    double need[3];
    for (int d = 0; d < 3; ++d)
        need[d] = hi[d] >= lo[d] ? (floor(hi[d]) - floor(lo[d]) + 2) / double(1 << gb[d]) : 1.0;
    int best[3] = {period_bits(w->group, 0), period_bits(w->group, 1), period_bits(w->group, 2)};
    best_period_split(PeriodSet(std::move(occ)), need, lg, best);
    const int32_t g = with_period(w->group, best[0], best[1], best[2]);
    if (g != w->group) {
        w->group = g;
        drop_graphs(w);                                  // the grid is a captured kernel argument
    }
    w->fit_key[6] = (int64_t)w->group;
}

}  // namespace rb::host

using namespace rb::host;

extern "C" {

int rb_set_state(rb_world *w, const double *qpos, const double *qvel) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w || !qpos || !qvel) return fail(RB_EINVAL, "null argument");
    HIPCHK(hipSetDevice(w->device));
    if (int rc = finish_pending(w)) return rc;
    if (int rc = io_alloc(w)) return rc;
    const size_t nq = (size_t)7 * w->N, nv = (size_t)6 * w->N;
    // the state the last rb_get_state handed out, handed back unchanged (a
    // per-frame caller: multi_sphere_bounce.py:42 once per frame): nothing
    // to do (one rank: a shard's rows of other ranks are not mirrored)
    if (w->P == 1 && w->mirror_version == w->state_version && par_equal2(qpos, w->io_q_h, nq, qvel, w->io_v_h, nv)) {
        w->io_stats[0] += 1;
        return RB_OK;
    }
    w->io_stats[1] += 1;
    HIPCHK(hipStreamSynchronize(w->stream));     // (a DMA out of the staging may be in flight)
    par_copy2(w->io_q_h, qpos, nq, w->io_v_h, qvel, nv);
    fit_period(w, qpos);
    HIPCHK(hipMemcpyAsync(w->io_q_d, w->io_q_h, sizeof(double) * nq, hipMemcpyHostToDevice, w->stream));
    HIPCHK(hipMemcpyAsync(w->io_v_d, w->io_v_h, sizeof(double) * nv, hipMemcpyHostToDevice, w->stream));
    const hipError_t e = by_real(w->dtype, [&](auto t) {
        using T = decltype(t);
        return launch_state_in<T>(make_io<T>(w), w->stream);
    });
    HIPCHK(e);
    w->primed = false;
    w->tile_valid_sp = -1;
    w->tile_fit_valid = false;                           // (refitted at the next tile run)
    if (w->tile_mode_init == -1 && w->tile_mode == 0) {   // a new state: auto mode may try the form again
        w->tile_mode = -1;
        w->tile_backoff = w->tile_skip = 0;
    }
    w->state_version += 1;
    // uploading the staging's bytes yields exactly this state (one rank)
    w->mirror_version = w->P == 1 ? w->state_version : -1;
    return RB_OK;
}

int rb_get_state(rb_world *w, double *qpos, double *qvel) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w || (!qpos && !qvel)) return fail(RB_EINVAL, "null argument");
    HIPCHK(hipSetDevice(w->device));
    if (int rc = finish_pending(w)) return rc;
    if (int rc = io_alloc(w)) return rc;
    // the owned rows only (a shard leaves the others untouched).  Default
    // (RBHIP_IO_OUT=2): one kernel stores the rows straight into the mapped
    // pinned staging (no DMA), then one pool copy out to the caller.  =0: a
    // kernel transposes into the device twin, one DMA, one pool copy; =1:
    // that DMA in four chunks, each copied out as it lands.  65,536 bodies
    // into the caller's arrays, MI355X: 0.21 / 0.22 / 0.28 ms for 2 / 0 / 1
    // (profiles/r04/frame_cost_16threads.log)
    const char *ev = getenv("RBHIP_IO_OUT");
    const int mode = ev ? atoi(ev) : 2;
    const size_t lo = (size_t)w->lo, n = (size_t)w->n_local;
    const size_t nq = qpos ? 7 * n : 0, nv = qvel ? 6 * n : 0;
    if (mode == 2) {
        HIPCHK(by_real(w->dtype, [&](auto t) {
            using T = decltype(t);
            StateIO<T> p = make_io<T>(w);
            p.qpos = w->io_q_h.dev();
            p.qvel = w->io_v_h.dev();
            return launch_state_out_flat<T>(p, qpos, qvel, w->stream);
        }));
        HIPCHK(hipStreamSynchronize(w->stream));
        par_copy2(qpos ? qpos + 7 * lo : nullptr, w->io_q_h + 7 * lo, nq, qvel ? qvel + 6 * lo : nullptr,
                  w->io_v_h + 6 * lo, nv);
    } else {
        HIPCHK(by_real(w->dtype, [&](auto t) {
            using T = decltype(t);
            return launch_state_out<T>(make_io<T>(w), qpos, qvel, w->stream);
        }));
        const int nc = mode == 1 && n >= 16384 ? 4 : 1;
        if (nc > 1 && !w->io_ev[0])
            for (hipEvent_t &e : w->io_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (int c = 0; c < nc; ++c) {
            const size_t a = lo + n * c / nc, b = lo + n * (c + 1) / nc;
            if (qpos) HIPCHK(hipMemcpyAsync(w->io_q_h + 7 * a, w->io_q_d + 7 * a, sizeof(double) * 7 * (b - a), hipMemcpyDeviceToHost, w->stream));
            if (qvel) HIPCHK(hipMemcpyAsync(w->io_v_h + 6 * a, w->io_v_d + 6 * a, sizeof(double) * 6 * (b - a), hipMemcpyDeviceToHost, w->stream));
            if (nc > 1) HIPCHK(hipEventRecord(w->io_ev[c], w->stream));
        }
        for (int c = 0; c < nc; ++c) {
            const size_t a = lo + n * c / nc, b = lo + n * (c + 1) / nc;
            if (nc > 1) HIPCHK(hipEventSynchronize(w->io_ev[c]));
            else HIPCHK(hipStreamSynchronize(w->stream));
            par_copy2(qpos ? qpos + 7 * a : nullptr, w->io_q_h + 7 * a, qpos ? 7 * (b - a) : 0,
                      qvel ? qvel + 6 * a : nullptr, w->io_v_h + 6 * a, qvel ? 6 * (b - a) : 0);
        }
    }
    w->mirror_version = (w->P == 1 && qpos && qvel) ? w->state_version : -1;
    return RB_OK;
}

}  // extern "C"
