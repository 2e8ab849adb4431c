// rb_api_tiles.hip — the host side of the cell-ordered tile form (kernels in
// rb_tiles.hip): the fit, the bins, the runs and their check.
#include "rb_host.hpp"

namespace rb::host {

bool tile_eligible(const rb_world *w) {
    if (w->tile_mode == 0 || w->tile_replaying || w->P != 1 || !w->all_spheres || w->law != RB_LAW_MUJOCO || w->xfrc || w->timing)
        return false;
    // (more than TILE_TYPES distinct (m, I): the hashed forms, which read them by id)
    if (w->maxp > 32 || w->n_local <= 0 || w->N > (int64_t)TILE_ID_MASK + 1 || w->tile_ntypes < 1) return false;
    return w->tile_mode == 1 || w->n_local >= w->tile_min_bodies;
}

// The tile grid from body positions (x, y at pos[k * stride], pos[k * stride + 1]):
// columns of the hashed cell size; tc columns per tile edge so that a tile
// holds ~80 bodies on average (a slot steps at most TILE_THREADS) and none
// holds more than 7/8 of that limit at the fit; ntx x nty slots covering the
// scene's extent plus a margin (periodic: a scene that outgrows it folds
// onto itself, which stays exact).
static void tile_fit(rb_world *w, const double *pos, int64_t stride) {
    const double inv = w->inv_cs;
    std::vector<int64_t> cols;
    cols.reserve((size_t)w->N);
    int64_t lo[2] = {INT64_MAX, INT64_MAX}, hi[2] = {INT64_MIN, INT64_MIN};
    for (int64_t b = 0; b < w->N; ++b) {
        const double fx = pos[b * stride] * inv, fy = pos[b * stride + 1] * inv;
        if (!(fabs(fx) < 1e9 && fabs(fy) < 1e9)) continue;
        const int64_t cx = (int64_t)floor(fx), cy = (int64_t)floor(fy);
        lo[0] = std::min(lo[0], cx); hi[0] = std::max(hi[0], cx);
        lo[1] = std::min(lo[1], cy); hi[1] = std::max(hi[1], cy);
        cols.push_back(((cx + (1 << 30)) << 31) | (cy + (1 << 30)));
    }
    if (cols.empty()) { lo[0] = lo[1] = 0; hi[0] = hi[1] = 0; }
    std::sort(cols.begin(), cols.end());
    const int64_t nocc = std::max<int64_t>(1, (int64_t)(std::unique(cols.begin(), cols.end()) - cols.begin()));
    const double per_col = (double)std::max<int64_t>(1, (int64_t)cols.size()) / (double)nocc;
    int tc = (int)lround(sqrt(80.0 / per_col));
    tc = std::max(TILE_TC_MIN, std::min(TILE_TC_MAX, tc));
    if (const char *ev = getenv("RBHIP_TILE_COLS")) tc = std::max(TILE_TC_MIN, std::min(TILE_TC_MAX, atoi(ev)));
    // the densest tile at this fit under 3/4 of a slot's limit
    for (; tc > TILE_TC_MIN; --tc) {
        std::vector<int64_t> t;
        t.reserve(cols.size());
        for (int64_t b = 0; b < w->N; ++b) {
            const double fx = pos[b * stride] * inv, fy = pos[b * stride + 1] * inv;
            if (!(fabs(fx) < 1e9 && fabs(fy) < 1e9)) continue;
            const int64_t tx = (int64_t)floor(floor(fx) / tc), ty = (int64_t)floor(floor(fy) / tc);
            t.push_back(((tx + (1 << 30)) << 31) | (ty + (1 << 30)));
        }
        std::sort(t.begin(), t.end());
        int64_t worst = 0;
        for (size_t a = 0; a < t.size();) {
            size_t e = a;
            while (e < t.size() && t[e] == t[a]) ++e;
            worst = std::max<int64_t>(worst, (int64_t)(e - a));
            a = e;
        }
        if (worst <= 7 * TILE_THREADS / 8) break;
    }
    int64_t ntx = (hi[0] - lo[0]) / tc + 3, nty = (hi[1] - lo[1]) / tc + 3;
    // a scene spread far (outliers): fold instead of launching empty slots
    const int64_t max_slots = 4 * ((w->N + 23) / 24) + 64;
    while (ntx * nty > max_slots) {
        if (ntx >= nty) ntx = (ntx + 1) / 2; else nty = (nty + 1) / 2;
    }
    w->tile_tc = tc;
    w->tile_ntx = (int32_t)std::max<int64_t>(3, ntx);
    w->tile_nty = (int32_t)std::max<int64_t>(3, nty);
    w->tile_fit_valid = true;
}

static size_t tile_bins_bytes(const rb_world *w) {
    const size_t slots = (size_t)w->tile_ntx * w->tile_nty, cap = (size_t)w->tile_cap, esz = (size_t)w->esz;
    return slots * TILE_OFFW * 4 + slots * cap * (4 * esz + 4 + TILE_STW * esz) + 256 +
           (size_t)TILE_FARMAX * (4 * esz + 4 + TILE_STW * esz) + 256;
}
template <typename T> static TileBins<T> tile_bins(const rb_world *w, int sp) {
    const size_t slots = (size_t)w->tile_ntx * w->tile_nty, cap = (size_t)w->tile_cap;
    char *b = static_cast<char *>(w->tile_mem.get()) + (size_t)sp * tile_bins_bytes(w);
    TileBins<T> t;
    t.off = reinterpret_cast<int32_t *>(b);
    b += slots * TILE_OFFW * 4;
    t.pos = reinterpret_cast<Snap<T> *>(b);
    b += slots * cap * 4 * sizeof(T);
    t.st = reinterpret_cast<T *>(b);
    b += slots * cap * TILE_STW * sizeof(T);
    t.id = reinterpret_cast<int32_t *>(b);
    b += (slots * cap * 4 + 255) / 256 * 256;
    t.far_hdr = reinterpret_cast<unsigned long long *>(b);
    b += 256;
    t.far_pos = reinterpret_cast<Snap<T> *>(b);
    b += (size_t)TILE_FARMAX * 4 * sizeof(T);
    t.far_st = reinterpret_cast<T *>(b);
    b += (size_t)TILE_FARMAX * TILE_STW * sizeof(T);
    t.far_id = reinterpret_cast<int32_t *>(b);
    return t;
}

// tile_build / tile_alloc: the auto mode's bins would not fit (a scene spread
// far, folded onto many mostly empty slots, or device memory short): the
// world steps hashed from now on (TILE_DECLINED)
constexpr size_t TILE_AUTO_MAX_BYTES_PER_BODY = 2048;   // flat scenes need ~0.4 KB

// the words the pending tile runs' checks read
static int tile_alloc_words(rb_world *w) {
    if (w->tile_gen) return RB_OK;
    WCHK(w->tile_gen.alloc(2 * sizeof(uint32_t)));
    WCHK(w->tile_why.alloc(sizeof(int32_t)));
    WCHK(w->tile_commits.alloc(sizeof(unsigned long long)));
    WCHK(wfill(w, w->tile_why, 0, sizeof(int32_t)));
    WCHK(wfill(w, w->tile_commits, 0, sizeof(unsigned long long)));
    WCHK(w->tile_host.alloc(4 * sizeof(int64_t)));
    WCHK(w->tile_pub_host.alloc(2 * sizeof(int64_t), hipHostMallocMapped | hipHostMallocCoherent));
    w->tile_commits_seen = 0;
    return RB_OK;
}

// Auto mode retires the tile form (a roll-back, or bins it will not
// allocate): the bins go too (hundreds of MB at millions of bodies), and the
// graphs that captured their pointers
static int tile_retire(rb_world *w) {
    w->tile_mode = 0;
    w->tile_valid_sp = -1;
    if (!w->tile_mem && !w->tile_fill) return RB_OK;
    HIPCHK(hipStreamSynchronize(w->stream));
    drop_graphs(w);
    w->tile_mem.reset();
    w->tile_fill.reset();
    return RB_OK;
}

static int tile_alloc(rb_world *w) {
    const size_t need = 2 * tile_bins_bytes(w);
    const size_t slots = (size_t)w->tile_ntx * w->tile_nty;
    if (w->tile_mem && w->tile_mem.bytes >= need && w->tile_fill) return RB_OK;   // (the fill scratch is sized for the slots too)
    if (w->tile_mode == -1 && need > TILE_AUTO_MAX_BYTES_PER_BODY * (size_t)w->N) {
        if (int rc = tile_retire(w)) return rc;
        return TILE_DECLINED;
    }
    HIPCHK(hipStreamSynchronize(w->stream));
    drop_graphs(w);                                  // captured bin pointers
    w->tile_mem.reset();
    w->tile_fill.reset();
    if (w->tile_mem.alloc(need) || w->tile_fill.alloc(slots * TILE_OFFW * 4)) {
        (void)hipGetLastError();
        w->tile_mem.reset();
        w->tile_fill.reset();
        if (w->tile_mode == -1) {
            if (int rc = tile_retire(w)) return rc;
            return TILE_DECLINED;
        }
        return fail(RB_ENOMEM, "tile bins: hipMalloc of %zu bytes failed", need);
    }
    return tile_alloc_words(w);
}

template <typename T> static TileIO<T> make_tile_io(rb_world *w, int64_t c) {
    w->err_pub = false;
    TileIO<T> p{};
    const int sp = (int)(c % 2);
    p.bins = tile_bins<T>(w, sp);
    p.gen = w->tile_gen + sp;
    p.snap = dp<Snap<T>>(w->snap[sp], 0);
    p.st = BodyState<T>{dp<T>(w->state, 0), w->S};
    p.fill = w->tile_fill;
    p.type_of = w->tile_type_of;
    p.tc = w->tile_tc; p.ntx = w->tile_ntx; p.nty = w->tile_nty; p.cap = w->tile_cap;
    p.inv_col = (T)w->inv_cs;
    p.n = w->N;
    p.err = w->err;
    p.why = w->tile_why;
    p.commits = w->tile_commits;
    return p;
}

template <typename T> static TileParams<T> make_tile_step(rb_world *w, int64_t c, double dt, double e, double mu, double thr) {
    w->err_pub = false;
    TileParams<T> p{};
    const int sp = (int)(c % 2);
    p.cur = tile_bins<T>(w, sp);
    p.next = tile_bins<T>(w, 1 - sp);
    p.gen_cur = w->tile_gen + sp;
    p.gen_next = w->tile_gen + (1 - sp);
    p.sp = make_step<T>(w, c, dt, e, mu, thr, false);
    p.ntypes = w->tile_ntypes;
    for (int t = 0; t < w->tile_ntypes; ++t)
        for (int k = 0; k < 4; ++k) p.types[t][k] = (T)w->tile_type_val[t][k];
    p.tc = w->tile_tc; p.ntx = w->tile_ntx; p.nty = w->tile_nty; p.cap = w->tile_cap;
    p.inv_col = (T)w->inv_cs;
    p.why = w->tile_why;
    return p;
}

// the bins of step c from the id-ordered state (snapshot and state rows)
static int tile_build(rb_world *w) {
    if (!w->tile_fit_valid) {
        // positions: the staging when it mirrors the state, else the snapshot
        if (w->io_q_h && w->mirror_version == w->state_version) {
            tile_fit(w, w->io_q_h, 7);
        } else {
            std::vector<double> q;
            WCHK(snapshot_to_host(w, q));
            tile_fit(w, q.data(), 4);
        }
        drop_graphs(w);                              // the grid is a captured kernel argument
    }
    if (int rc = tile_alloc(w)) return rc;
    const int sp = w->sp();
    const size_t slots = (size_t)w->tile_ntx * w->tile_nty;
    HIPCHK(hipMemsetAsync(w->tile_fill, 0, slots * TILE_OFFW * 4, w->stream));
    const int rc = by_real(w->dtype, [&](auto t) -> int {
        using T = decltype(t);
        for (int k = 0; k < 2; ++k)                  // far lists empty (tag 0: never a live generation)
            HIPCHK(hipMemsetAsync(tile_bins<T>(w, k).far_hdr, 0, sizeof(unsigned long long), w->stream));
        HIPCHK(hipMemsetAsync(tile_bins<T>(w, sp).off, 0, slots * TILE_OFFW * 4, w->stream));
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(w->tile_gen + sp), 1, 1, w->stream));
        HIPCHK(launch_tile_build<T>(make_tile_io<T>(w, w->c), w->stream));
        return RB_OK;
    });
    if (rc) return rc;
    w->tile_valid_sp = sp;
    w->tile_stats[3] += 1;
    return RB_OK;
}

// One run of n tile steps from step c (graph-replayed in chunks; the last
// chunk ends with the unbin kernel), recorded as pending until checked.
int tile_run(rb_world *w, int64_t n, double dt, double e, double mu, double thr) {
    if (w->tile_valid_sp != w->sp()) {
        if (int rc = finish_pending(w)) return rc;  // (the build reads the id-ordered state)
        if (int rc = tile_build(w)) return rc;
    }
    const int64_t c0 = w->c, chunk_max = 512;
    int64_t left = n;
    while (left > 0) {
        const int64_t K = left > chunk_max ? chunk_max : left;
        const bool last = K == left;
        const int variant = 16 | (int)w->record | (last ? 32 : 0);
        int rc = graph_replay(w, K, variant, dt, e, mu, thr, [&](hipStream_t s, int64_t cs) {
            return by_real(w->dtype, [&](auto t) -> int {
                using T = decltype(t);
                for (int64_t k = 0; k < K; ++k)
                    HIPCHK(launch_tile_step<T>(make_tile_step<T>(w, cs + k, dt, e, mu, thr), w->maxp, s));
                if (last) HIPCHK(launch_tile_unbin<T>(make_tile_io<T>(w, cs + K), s));
                return RB_OK;
            });
        });
        if (rc) return rc;
        w->c += K;
        left -= K;
    }
    w->tile_valid_sp = w->sp();
    w->primed = false;                               // the hashed forms' table is stale
    w->tile_pending.push_back(rb_world::TileRun{c0, n, dt, e, mu, thr});
    w->tile_stats[0] += 1;
    return RB_OK;
}

// The check of the pending tile runs: every run whose unbin committed is
// done; the first run that raised ERR_TILE and every run after it are
// replayed, from the id-ordered state (which still holds that run's start),
// by the hashed-cell forms — which report any real error themselves.
int tile_finish(rb_world *w) {
    if (w->tile_pending.empty()) return RB_OK;
    int32_t err, why;
    unsigned long long commits;
    if (w->err_pub && w->tile_pub) {
        // the last tile graph published the three words (publish_err_kernel)
        HIPCHK(hipStreamSynchronize(w->stream));
        err = __atomic_load_n(w->err_host.get(), __ATOMIC_ACQUIRE);
        why = (int32_t)__atomic_load_n(w->tile_pub_host.get(), __ATOMIC_ACQUIRE);
        commits = (unsigned long long)__atomic_load_n(w->tile_pub_host + 1, __ATOMIC_ACQUIRE);
    } else {
        HIPCHK(hipMemcpyAsync(w->tile_host, w->err, sizeof(int32_t), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(hipMemcpyAsync(w->tile_host + 1, w->tile_why, sizeof(int32_t), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(hipMemcpyAsync(w->tile_host + 2, w->tile_commits, sizeof(unsigned long long), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(hipStreamSynchronize(w->stream));
        err = (int32_t)reinterpret_cast<int32_t *>(w->tile_host.get())[0];
        why = (int32_t)reinterpret_cast<int32_t *>(w->tile_host + 1)[0];
        commits = (unsigned long long)w->tile_host[2];
    }
    const size_t ok = (size_t)(commits - w->tile_commits_seen);
    w->tile_commits_seen = commits;
    std::vector<rb_world::TileRun> runs;
    runs.swap(w->tile_pending);
    for (size_t k = 0; k < ok && k < runs.size(); ++k) w->tile_stats[1] += runs[k].n;
    if (!(err & ERR_TILE)) {
        if (w->tile_backoff > 0) w->tile_backoff /= 2;
        return RB_OK;
    }
    // roll back to the start of the first failed run and replay it and
    // every later one with the hashed-cell forms (guarded chunks: the
    // replay grows max_partners or refits the table as a synchronous
    // rb_step would)
    const size_t first = std::min(ok, runs.size());
    const int32_t clean = err & ~ERR_TILE;
    w->err_pub = false;
    HIPCHK(hipMemcpyAsync(w->err, &clean, sizeof(int32_t), hipMemcpyHostToDevice, w->stream));
    HIPCHK(hipMemsetAsync(w->tile_why, 0, sizeof(int32_t), w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    w->tile_valid_sp = -1;
    w->primed = false;
    w->tile_stats[2] += 1;
    w->tile_why_seen |= why;
    if (why & (TILE_WHY_CAP | TILE_WHY_WINDOW)) w->tile_fit_valid = false;   // the scene outgrew the fit
    w->tile_backoff = w->tile_backoff ? std::min(2 * w->tile_backoff, 64) : 1;
    w->tile_skip = w->tile_backoff;
    // auto mode: a scene that outgrew the tile slots once (pile-ups) tends to
    // keep doing so, and every retry costs a roll-back — step hashed from now on
    if (w->tile_mode == -1)
        if (int rc = tile_retire(w)) return rc;
    w->c = first < runs.size() ? runs[first].c0 : w->c;
    const bool saved = w->sync_call;
    w->sync_call = true;
    w->tile_replaying = true;
    int rc = RB_OK;
    for (size_t k = first; k < runs.size() && !rc; ++k) {
        const rb_world::TileRun &r = runs[k];
        rc = enqueue_steps(w, r.n, r.dt, r.e, r.mu, r.thr, false);
    }
    w->tile_replaying = false;
    w->sync_call = saved;
    return rc;
}

}  // namespace rb::host
