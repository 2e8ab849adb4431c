// rb_api_step.hip — stepping: the step kernels' parameters, the table's
// prime, the captured-graph cache, the chunks of a run (the guarded ones:
// rb_api_guard.hip), and rb_step / rb_step_async / rb_sync.
#include "rb_host.hpp"

namespace rb::host {

// Append epochs: sphere-only worlds on one rank (no exchange, whose ghosts
// need an insert per step) under the default law, stepped by a wide form.
bool epoch_eligible(const rb_world *w) {
    const int form = step_form(w);
    return w->epoch_max > 1 && w->ep_mem && w->P == 1 && !w->p2p && !w->comm && w->all_spheres && !w->boxes &&
           w->law == RB_LAW_MUJOCO && !w->plist && (form == FORM_WIDE || form == FORM_WIDE_HELP);   // (plist: the split form)
}

template <typename T> static Grid<T> make_grid(const rb_world *w) {
    Grid<T> g;
    g.inv_cs = (T)w->inv_cs;
    g.hmask = (uint32_t)(w->H - 1);
    g.H = (int32_t)w->H;
    g.super = w->group;
    return g;
}

// the broadphase of the steps of parity sp
template <typename T> static Table<T> table(const rb_world *w, int sp) {
    return Table<T>{w->ids[sp], w->pos[sp] ? dp<Snap<T>>(w->pos[sp], 0) : nullptr, w->gen + sp, w->spill[sp]};
}

// parameters of the step with counter value c
template <typename T> StepParams<T> make_step(rb_world *w, int64_t c, double dt, double e, double mu, double thr,
                                              bool insert_next) {
    w->err_pub = false;
    StepParams<T> p{};
    p.n_global = w->N;
    p.n_local = w->n_local;
    p.lo = (int32_t)w->lo;
    p.S = (int32_t)w->S;
    p.st.base = dp<T>(w->state, 0);
    p.st.S = w->S;
    p.cs.base = dp<T>(w->consts, 0);
    p.cs.Npad = w->Npad;
    p.cs.kind = w->kind;
    p.xfrc = w->xfrc ? dp<T>(w->xfrc, 0) : nullptr;
    p.n_planes = w->n_planes;
    for (int k = 0; k < w->n_planes; ++k)
        for (int d = 0; d < 3; ++d) { p.pn[k][d] = (T)w->planes[k][d]; p.pp[k][d] = (T)w->planes[k][3 + d]; }
    for (int d = 0; d < 3; ++d) p.g[d] = (T)w->g[d];
    p.dt = (T)dt; p.e = (T)e; p.mu = (T)mu; p.thr = (T)thr;
    p.oriented = w->oriented;
    p.grid = make_grid<T>(w);
    const int sp = (int)(c % 2);
    p.snap_cur = dp<Snap<T>>(w->snap[sp], 0);
    p.snap_next = dp<Snap<T>>(w->snap[1 - sp], 0);
    p.cur = table<T>(w, sp);
    p.next = insert_next ? table<T>(w, 1 - sp) : Table<T>{nullptr, nullptr, nullptr, nullptr};
    p.err = w->err;
    p.epoch = w->p2p ? w->epoch : nullptr;
    p.bounds = w->p2p ? w->bounds + (c % 2) * BOUND_COPIES * BOUND_STRIDE : nullptr;   // (peer-to-peer: both modes filter by them)
    if (w->p2p && w->halo) {                     // the step kernels push to the peers (rb_halo.hpp)
        p.halo.peer_mail = reinterpret_cast<char *const *>(w->peer_flags_dev.get());
        p.halo.mail = reinterpret_cast<const char *>(w->flags.get());
        p.halo.push_cnt = w->push_cnt;
        p.halo.halo_e = w->halo_e;
        p.halo.lay = MailLayout::make(w->P, w->S, w->esz, w->boxes);
        p.halo.S = w->S;
        p.halo.timeout_ticks = 500000000;        // 5 s at 100 MHz
        p.halo.rank = (int32_t)w->rank;
        p.halo.P = (int32_t)w->P;
    }
    p.plist = w->plist;
    p.plist_cnt = w->plist_cnt;
    if (w->vel[0]) {
        p.vel_cur = dp<Vel<T>>(w->vel[sp], 0);
        p.vel_next = dp<Vel<T>>(w->vel[1 - sp], 0);
    }
    p.tol = (T)w->tol;
    p.ground = w->n_planes > 0;
    if (w->boxes) {
        p.quat_cur = dp<T>(w->qsnap[sp], 0);
        p.quat_next = dp<T>(w->qsnap[1 - sp], 0);
        p.defer_q = w->defer_q;
        p.defer_cnt = w->defer_cnt + sp;
        p.defer_reset = w->defer_cnt + (1 - sp);
    }
    if (w->record) {
        p.rec_count = w->rec_count; p.rec_partner = w->rec_partner; p.rec_kind = w->rec_kind;
        p.rec_dist = dp<T>(w->rec_dist, 0);
        p.maxrec = w->maxrec;
    }
    if (insert_next && epoch_eligible(w)) {
        int32_t *crowd = reinterpret_cast<int32_t *>(w->ep_mem + 2);
        p.ep.ctrl = w->ep_ctrl() + sp;
        p.ep.ctrl_next = w->ep_ctrl() + (1 - sp);
        for (int k = 0; k < 2; ++k) { p.ep.line[k] = w->ids[k]; p.ep.spill[k] = w->spill[k]; }
        p.ep.crowd = crowd + sp;
        p.ep.crowd_prev = crowd + (1 - sp);
        p.ep.count = reinterpret_cast<unsigned long long *>(w->ep_mem + 4);
        p.ep.len_max = w->epoch_max;
    }
    return p;
}

template <typename T> InsertParams<T> make_insert(rb_world *w, int sp, int64_t first, int64_t count,
                                                  int64_t skip_lo, int64_t skip_hi) {
    w->err_pub = false;
    InsertParams<T> ip{};
    ip.snap = dp<Snap<T>>(w->snap[sp], 0);
    ip.kind = w->kind;
    ip.first = first; ip.count = count; ip.skip_lo = skip_lo; ip.skip_hi = skip_hi;
    ip.grid = make_grid<T>(w);
    ip.tab = table<T>(w, sp);
    ip.err = w->err;
    return ip;
}

// (the tile and sharding units build on these two)
template StepParams<double> make_step<double>(rb_world *, int64_t, double, double, double, double, bool);
template StepParams<float> make_step<float>(rb_world *, int64_t, double, double, double, double, bool);
template InsertParams<double> make_insert<double>(rb_world *, int, int64_t, int64_t, int64_t, int64_t);
template InsertParams<float> make_insert<float>(rb_world *, int, int64_t, int64_t, int64_t, int64_t);

// (re)build the current table from every body's snapshot; under the
// two-ball law first run the coming step's ground phase from the true state
// (it depends on dt, e, mu: remembered, and re-primed when they change)
int prime(rb_world *w, double dt, double e, double mu) {
    if (w->law == RB_LAW_BALLS) {
        const hipError_t r = by_real(w->dtype, [&](auto t) {
            using T = decltype(t);
            StepParams<T> p = make_step<T>(w, w->c, dt, e, mu, 0.0, false);
            p.snap_next = dp<Snap<T>>(w->snap[w->sp()], 0);
            p.vel_next = dp<Vel<T>>(w->vel[w->sp()], 0);
            return launch_ball_prime<T>(p, w->stream);
        });
        HIPCHK(r);
        w->prm_dt = dt; w->prm_e = e; w->prm_mu = mu;
    }
    // a fresh table: a generation above every one used so far
    w->gen_off += 1;
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(w->gen + w->sp()), (int)(w->gen_off + (uint32_t)w->c), 1, w->stream));
    const hipError_t ie = by_real(w->dtype, [&](auto t) {
        using T = decltype(t);
        return launch_insert<T>(make_insert<T>(w, w->sp(), 0, w->N, 0, 0), w->stream);
    });
    HIPCHK(ie);
    // a fresh epoch: the step reads the table just built (the one of its
    // parity); the crowding flags of any epoch cut short are dropped
    w->ep_primed = epoch_eligible(w);
    if (w->ep_primed) {
        const uint32_t cw = epoch_word((uint32_t)w->sp(), 0u, std::min((uint32_t)w->epoch_max, EP_START_LEN), false, 0u);
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(w->ep_ctrl() + w->sp()), (int)cw, 1, w->stream));
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(w->ep_mem + 2), 0, 2, w->stream));
    }
    w->primed = true;
    return RB_OK;
}

// the per-step kernel form of this world (a world keeps it; a switch of
// form would have to re-prime: the epoch schedule belongs to the wide forms)
int step_form(const rb_world *w) {
    return w->n_local <= w->coop_max ? (w->n_local <= w->help_max ? FORM_COOP_HELP : FORM_COOP)
           : w->n_local <= w->wide_max ? (w->wide_help ? FORM_WIDE_HELP : FORM_WIDE) : FORM_ONE;
}

int launch_one(rb_world *w, hipStream_t s, int64_t c, double dt, double e, double mu, double thr) {
    const int form = step_form(w);
    const bool boxes = w->boxes && w->box_kernel_on;
    const hipError_t r = by_real(w->dtype, [&](auto t) {
        using T = decltype(t);
        const StepParams<T> p = make_step<T>(w, c, dt, e, mu, thr, true);
        return w->law == RB_LAW_BALLS ? launch_ball_step<T>(p, w->maxp, s) : launch_step<T>(p, w->maxp, form, boxes, w->help_search, s);
    });
    HIPCHK(r);
    return RB_OK;
}

static int read_err(rb_world *w) {
    // the word reaches pinned host memory through publish_err_kernel: at the
    // end of the last graph, or enqueued here when other error-writing work
    // followed it (a separate launch costs ~9 us at a sync)
    if (!w->err_pub) HIPCHK(launch_publish_err(w->err, w->err_host.dev(), w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    const int32_t bits = __atomic_load_n(w->err_host.get(), __ATOMIC_ACQUIRE);
    if (bits) {
        w->err_pub = false;
        HIPCHK(hipMemsetAsync(w->err, 0, sizeof(int32_t), w->stream));
        HIPCHK(hipStreamSynchronize(w->stream));
        return err_to_code(bits);
    }
    return RB_OK;
}

int collect_timing(rb_world *w) {
    if (w->tev.empty()) return RB_OK;
    HIPCHK(hipStreamSynchronize(w->stream));
    for (auto &pr : w->tev) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, pr.first, pr.second));
        w->t_sum_ms += ms;
        w->t_n += 1;
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    w->tev.clear();
    return RB_OK;
}

int timed_launch(rb_world *w, double dt, double e, double mu, double thr) {
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    HIPCHK(hipEventRecord(a, w->stream));
    int rc = launch_one(w, w->stream, w->c, dt, e, mu, thr);
    if (rc) return rc;
    HIPCHK(hipEventRecord(b, w->stream));
    w->tev.emplace_back(a, b);
    if (w->tev.size() >= 4096) return collect_timing(w);
    return RB_OK;
}

void drop_graphs(rb_world *w) {
    for (auto &kv : w->graphs) (void)hipGraphExecDestroy(kv.second.ex);
    w->graphs.clear();
}

constexpr size_t GRAPH_CACHE_MAX = 32;

// evict least recently used graphs until `room` more fit
static void evict_graphs(rb_world *w, size_t room) {
    while (!w->graphs.empty() && w->graphs.size() + room > GRAPH_CACHE_MAX) {
        auto lru = w->graphs.begin();
        for (auto it = w->graphs.begin(); it != w->graphs.end(); ++it)
            if (it->second.used < lru->second.used) lru = it;
        (void)hipGraphExecDestroy(lru->second.ex);
        w->graphs.erase(lru);
    }
}

// Table generations are 32-bit and only grow: before they would wrap (after
// ~4e9 steps of one world) the bucket lines are zeroed and the table
// rebuilt at generation 2 — from the snapshot, which holds every body's
// position except in a halo-exchanging shard (there: an error).
int gen_guard(rb_world *w, int64_t nsteps) {
    const uint64_t g = (uint32_t)(w->gen_off + (uint32_t)w->c);
    if (g + (uint64_t)nsteps + 4 < (1ull << 32)) return RB_OK;
    if (w->halo)
        return fail(RB_EOVERFLOW, "table generations exhausted after ~4e9 steps of a halo-exchanging shard: "
                                  "the sharded world must be recreated");
    HIPCHK(hipStreamSynchronize(w->stream));
    for (int k = 0; k < 2; ++k) {
        WCHK(wfill(w, w->ids[k], 0, line_bytes(w->H)));
        WCHK(wfill(w, w->spill[k], 0, spill_bytes));
    }
    w->gen_off = 1u - (uint32_t)w->c;   // prime() makes step c's generation 2
    w->primed = false;
    return RB_OK;
}

// ---- captured step graphs ---------------------------------------------------
// A sequence of launches covering K steps from step c0 (`seq(stream, c0)`),
// captured once per start parity and replayed (rb_world::graphs, keyed by the
// step count, parity, step parameters and variant).
int graph_replay(rb_world *w, int64_t K, int variant, double dt, double e, double mu, double thr,
                 const std::function<int(hipStream_t, int64_t)> &seq) {
    const bool tile_graph = (variant & 16) && w->tile_pub_host;   // (a tile run's: its words too)
    auto key = std::make_tuple(K, (int)(w->c % 2), dt, e, mu, thr, variant);
    auto it = w->graphs.find(key);
    if (it == w->graphs.end()) {
        evict_graphs(w, 2);
        // capture both parities at once, so later calls starting at either
        // replay without a capture (a parity still cached is kept; both
        // entries get the current tick, so the one not launched now is not
        // the first evicted).  No other thread inside the library meanwhile
        // (CaptureScope).
        CaptureScope capture_scope_;
        for (int c0 = 0; c0 < 2; ++c0) {
            const auto k0 = std::make_tuple(K, c0, dt, e, mu, thr, variant);
            auto old = w->graphs.find(k0);
            if (old != w->graphs.end()) { old->second.used = w->graph_tick; continue; }
            hipGraph_t graph;
            hipGraphExec_t ex;
            HIPCHK(hipStreamBeginCapture(w->cap_stream, hipStreamCaptureModeThreadLocal));
            int rc = seq(w->cap_stream, c0);
            const hipError_t pe = rc ? hipSuccess
                                     : tile_graph ? launch_publish_err(w->err, w->err_host.dev(), w->cap_stream, w->tile_why,
                                                                       w->tile_commits, w->tile_pub_host.dev())
                                                  : launch_publish_err(w->err, w->err_host.dev(), w->cap_stream);
            if (rc || pe != hipSuccess) {
                (void)hipStreamEndCapture(w->cap_stream, &graph);
                if (rc) return rc;
                HIPCHK(pe);
            }
            HIPCHK(hipStreamEndCapture(w->cap_stream, &graph));
            HIPCHK(hipGraphInstantiate(&ex, graph, nullptr, nullptr, 0));
            (void)hipGraphDestroy(graph);
            w->graphs[k0] = rb_world::GraphEntry{ex, w->graph_tick};
        }
        it = w->graphs.find(key);
    }
    it->second.used = ++w->graph_tick;
    HIPCHK(hipGraphLaunch(it->second.ex, w->stream));
    w->err_pub = true;                               // (the graph ends in publish_err_kernel)
    w->tile_pub = tile_graph;
    return RB_OK;
}

// nsteps steps (sharded: with the in-library exchange), graph-replayed
int enqueue_steps(rb_world *w, int64_t nsteps, double dt, double e, double mu, double thr, bool sharded) {
    if (nsteps < 0) return fail(RB_EINVAL, "nsteps < 0");
    if (!sharded && w->P != 1) return fail(RB_EINVAL, "rb_step on a sharded world: use rb_shard_run or rb_shard_step + exchange");
    if (sharded && !w->comm && !w->p2p) return fail(RB_EINVAL, "rb_shard_run before rb_shard_comm_init or rb_p2p_connect");
    if (sharded && w->law != RB_LAW_MUJOCO) return fail(RB_EUNSUPPORTED, "sharded stepping supports the default contact law only");
    if (!(dt > 0) || !(e >= 0) || !(mu >= 0) || !(thr >= 0))
        return fail(RB_EINVAL, "invalid step parameters dt=%g e=%g mu=%g thr=%g", dt, e, mu, thr);
    if (nsteps == 0) return RB_OK;
    HIPCHK(hipSetDevice(w->device));
    // the tile form for runs of >= 2 steps, or to continue from its bins;
    // pending tile runs chain (their check waits for the next sync point),
    // anything else first settles them
    const bool tile = !sharded && tile_eligible(w) && (nsteps >= 2 || w->tile_valid_sp == w->sp()) &&
                      w->tile_pending.size() < 256;
    if (tile && w->tile_skip > 0 && w->tile_valid_sp != w->sp()) {
        --w->tile_skip;                              // (back-off after a roll-back: this run steps hashed)
    } else if (tile) {
        w->state_version += 1;
        const int rc = tile_run(w, nsteps, dt, e, mu, thr);
        if (rc != TILE_DECLINED) return rc;          // (declined: the hashed forms below)
    }
    if (int rc = finish_pending(w)) return rc;
    w->state_version += 1;
    w->tile_valid_sp = -1;                           // the hashed forms advance the id-ordered state
    if (int rc = gen_guard(w, nsteps)) return rc;
    if (epoch_eligible(w) != w->ep_primed) w->primed = false;   // (the table a step reads: the epoch's, or its parity's)
    if (!w->primed || (w->law == RB_LAW_BALLS && (dt != w->prm_dt || e != w->prm_e || mu != w->prm_mu))) {
        int rc = prime(w, dt, e, mu);
        if (rc) return rc;
    }
    if (sharded && w->p2p && w->halo)
        if (int rc = halo_prime(w)) return rc;
    auto one = [&](hipStream_t s, int64_t c) {
        return sharded ? shard_one(w, s, c, dt, e, mu, thr) : launch_one(w, s, c, dt, e, mu, thr);
    };
    if (w->timing) {
        // eager launches, each step kernel bracketed by events on the launch stream
        for (int64_t k = 0; k < nsteps; ++k) {
            int rc = timed_launch(w, dt, e, mu, thr);
            if (!rc && sharded) rc = shard_exchange(w, w->stream, w->c);
            if (rc) return rc;
            ++w->c;
        }
        return RB_OK;
    }
    if (nsteps == 1) {
        int rc = one(w->stream, w->c);
        if (rc) return rc;
        ++w->c;
        return RB_OK;
    }
    // K > 1: replay a captured graph of K step nodes
    auto replay = [&](int64_t K, int variant) -> int {
        return graph_replay(w, K, variant, dt, e, mu, thr, [&](hipStream_t s, int64_t c0) {
            for (int64_t k = 0; k < K; ++k)
                if (int rc = one(s, c0 + k)) return rc;
            return (int)RB_OK;
        });
    };
    const int variant = (int)w->record | (sharded ? 2 : 0);
    const int64_t chunk_max = 512;
    const bool solo = !sharded && w->P == 1;                 // one rank, no exchange: chunks can be rolled back
    const bool box_chunks = w->boxes && w->box_opt && solo;  // box worlds' chunks run without the box kernel
    int64_t left = nsteps;
    while (left > 0) {
        int64_t K = left > chunk_max ? chunk_max : left;
        bool opt = box_chunks && w->box_skip == 0;
        // a chunk run with the box kernel because of an earlier roll-back
        // counts down the back-off (guarded or not)
        if (box_chunks && w->box_skip > 0) --w->box_skip;
        // a guarded chunk can be rolled back: optimistic box chunks, and long
        // chunks of a synchronous call (rb_step), whose broadphase layout is
        // refitted if the scene drifted out of it (a bucket overflowed)
        const bool guard = opt || (w->sync_call && K >= GUARD_MIN_STEPS && solo && w->law == RB_LAW_MUJOCO);
        const int rc = !guard ? replay(K, variant)
                              : guarded_chunk(w, K, left, opt, dt, e, mu, [&](int64_t k, bool o) { return replay(k, variant | (o ? 4 : 0)); });
        if (rc) return rc;
        w->c += K;
        left -= K;
    }
    return RB_OK;
}

}  // namespace rb::host

using namespace rb::host;

extern "C" {

int rb_step_async(rb_world *w, int64_t nsteps, double dt, double e, double mu, double thr) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w) return fail(RB_EINVAL, "null world");
    return enqueue_steps(w, nsteps, dt, e, mu, thr);
}

int rb_sync(rb_world *w) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w) return fail(RB_EINVAL, "null world");
    HIPCHK(hipSetDevice(w->device));
    if (int rc = finish_pending(w)) return rc;
    return read_err(w);
}

int rb_step(rb_world *w, int64_t nsteps, double dt, double e, double mu, double thr) {
    ApiScope api_scope_(w ? w->device : -1);
    if (w) w->sync_call = true;
    int rc = rb_step_async(w, nsteps, dt, e, mu, thr);
    if (w) w->sync_call = false;
    if (rc) return rc;
    if ((rc = finish_pending(w))) return rc;
    return read_err(w);
}

}  // extern "C"
