// rb_api_world.hip — a world's lifetime (rb_world_create with its environment
// switches, the constants' upload, rb_world_destroy), its small setters and
// its queries.
#include <array>

#include "rb_host.hpp"

using namespace rb::host;

namespace {

double bound_of(const rb_scene_desc *d, int64_t b) {
    const double *s = d->size + 3 * b;
    return d->kind[b] == RB_BODY_SPHERE ? s[0] : sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
}

template <typename T>
int upload_consts(rb_world *w, const rb_scene_desc *d, std::vector<double> &bound) {
    std::vector<T> c((size_t)8 * w->Npad, T(0));
    double rmax = 0;
    bound.assign((size_t)w->N, 0.0);
    for (int64_t b = 0; b < w->N; ++b) {
        const double *s = d->size + 3 * b;
        bound[(size_t)b] = bound_of(d, b);
        if (bound[(size_t)b] > rmax) rmax = bound[(size_t)b];
        c[(size_t)(0 * w->Npad + b)] = (T)d->mass[b];
        for (int k = 0; k < 3; ++k) {
            c[(size_t)((1 + k) * w->Npad + b)] = (T)d->inertia[3 * b + k];
            c[(size_t)((4 + k) * w->Npad + b)] = (T)s[k];
        }
        c[(size_t)(7 * w->Npad + b)] = (T)bound[(size_t)b];
    }
    // cell = 2 x the largest contact reach (2 x 2 rmax): the 2x2x2 query
    w->rmax = rmax;
    const double cs = rmax > 0 ? 4.0 * rmax * 1.001 : 1.0;
    w->inv_cs = 1.0 / cs;
    for (int64_t b = 0; b < w->N; ++b) w->all_spheres = w->all_spheres && d->kind[b] == RB_BODY_SPHERE;
    WCHK(wput(w, w->consts, c.data(), sizeof(T) * c.size()));
    // the tile form's constant types: the distinct (m, I) of the bodies, as
    // the arithmetic type holds them (a record carries its type, so the tile
    // kernel reads m and I from a table in LDS instead of by body id)
    {
        std::vector<std::array<T, 4>> types;
        std::vector<uint8_t> type_of((size_t)w->N, 0);
        for (int64_t b = 0; b < w->N && types.size() <= (size_t)TILE_TYPES; ++b) {
            const std::array<T, 4> t = {(T)d->mass[b], (T)d->inertia[3 * b], (T)d->inertia[3 * b + 1], (T)d->inertia[3 * b + 2]};
            size_t k = 0;
            while (k < types.size() && memcmp(types[k].data(), t.data(), sizeof(t)) != 0) ++k;
            if (k == types.size()) types.push_back(t);
            type_of[(size_t)b] = (uint8_t)k;
        }
        if (types.size() <= (size_t)TILE_TYPES) {
            for (size_t t = 0; t < types.size(); ++t)
                for (int k = 0; k < 4; ++k) w->tile_type_val[t][k] = (double)types[t][k];
            WCHK(w->tile_type_of.alloc((size_t)w->N));
            WCHK(wput(w, w->tile_type_of, type_of.data(), (size_t)w->N));
            w->tile_ntypes = (int32_t)types.size();
        }
    }
    std::vector<int32_t> k((size_t)w->Npad, 0);
    for (int64_t b = 0; b < w->N; ++b) k[(size_t)b] = d->kind[b];
    WCHK(wput(w, w->kind, k.data(), sizeof(int32_t) * k.size()));
    return RB_OK;
}

// Teardown: the graphs that captured the buffers, the communicator and the
// peers' mappings, the events; then every buffer, by its owner's destructor,
// with the world's device current; the two streams last
void free_world(rb_world *w) {
    if (!w) return;
    (void)hipSetDevice(w->device);
    drop_graphs(w);
    shard_release(w);
    for (auto &pr : w->tev) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (hipEvent_t &e : w->io_ev)
        if (e) (void)hipEventDestroy(e);
    const hipStream_t own_stream = w->own_stream, cap_stream = w->cap_stream;
    delete w;
    if (own_stream) (void)hipStreamDestroy(own_stream);
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
}

}  // namespace

extern "C" {

int rb_world_create(rb_world **out, const rb_scene_desc *d) {
    ApiScope api_scope_(d ? d->device : -1);
    if (!out || !d) return fail(RB_EINVAL, "null argument");
    *out = nullptr;
    if (d->n_bodies <= 0 || d->n_bodies > (int64_t)INT32_MAX / 2) return fail(RB_EINVAL, "n_bodies out of range");
    if (d->n_planes < 0 || d->n_planes > RB_MAX_PLANES) return fail(RB_EINVAL, "n_planes must be in [0, %d]", RB_MAX_PLANES);
    if (d->dtype != RB_F64 && d->dtype != RB_F32) return fail(RB_EINVAL, "dtype must be RB_F64 or RB_F32");
    if (d->world_size < 1 || d->rank < 0 || d->rank >= d->world_size) return fail(RB_EINVAL, "bad rank/world_size");
    if (!d->kind || !d->mass || !d->inertia || !d->size || (d->n_planes && !d->planes))
        return fail(RB_EINVAL, "null scene array");
    if (d->normal_convention != RB_NORMAL_ORIENTED && d->normal_convention != RB_NORMAL_RAW)
        return fail(RB_EINVAL, "bad normal_convention");
    const int maxp = d->max_partners > 0 ? d->max_partners : 16;
    if (maxp > 32) return fail(RB_EINVAL, "max_partners must be <= 32");
    if (d->bucket_capacity < 0 || d->bucket_capacity > BUCKET_SLOTS)
        return fail(RB_EINVAL, "bucket_capacity must be <= %d", BUCKET_SLOTS);
    for (int64_t b = 0; b < d->n_bodies; ++b) {
        if (d->kind[b] != RB_BODY_SPHERE && d->kind[b] != RB_BODY_BOX) return fail(RB_EINVAL, "body %lld: bad kind", (long long)b);
        if (!(d->mass[b] > 0)) return fail(RB_EINVAL, "body %lld: mass must be > 0", (long long)b);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(RB_ENODEV, "no HIP device available");
    if (d->device < 0 || d->device >= ndev) return fail(RB_ENODEV, "device %d out of range (have %d)", d->device, ndev);

    int64_t n_spheres = 0;
    for (int64_t b = 0; b < d->n_bodies; ++b) n_spheres += d->kind[b] == RB_BODY_SPHERE;
    const WorldCounts sc{d->n_bodies, d->world_size, d->rank, n_spheres != d->n_bodies, n_spheres, d->dtype == RB_F64 ? 8 : 4,
                         d->max_partners, d->n_planes};
    const WorldPlan plan = world_plan(sc, WorldSwitches::from_environ());

    rb_world *w = new rb_world();
    w->dtype = d->dtype;
    w->esz = sc.esz;
    w->device = d->device;
    w->N = sc.N;
    w->P = sc.P;
    w->rank = sc.rank;
    w->n_planes = d->n_planes;
    for (int k = 0; k < d->n_planes; ++k)
        for (int j = 0; j < 6; ++j) w->planes[k][j] = d->planes[6 * k + j];
    for (int j = 0; j < 3; ++j) w->g[j] = d->gravity[j];
    w->oriented = d->normal_convention == RB_NORMAL_ORIENTED;
    static_cast<WorldPlan &>(*w) = plan;
    w->tile_mode_init = w->tile_mode;

    auto bail = [&](int rc) { free_world(w); return rc; };
    if (hipSetDevice(w->device) != hipSuccess) return bail(fail(RB_ENODEV, "hipSetDevice(%d) failed", w->device));
    // (after a failure nothing more is allocated)
    int arc = RB_OK;
    auto alloc = [&](DevMem &b, size_t bytes) { if (!arc) arc = b.alloc(bytes); };
    for (int k = 0; k < 2; ++k) alloc(w->snap[k], snap_bytes(w));
    if (w->boxes) {
        for (int k = 0; k < 2; ++k) alloc(w->qsnap[k], snap_bytes(w));
        alloc(w->defer_q, sizeof(int32_t) * (w->S > 0 ? w->S : 1));
        alloc(w->defer_cnt, sizeof(int32_t) * 2);
    }
    alloc(w->state, state_bytes(w));
    alloc(w->consts, consts_bytes(w));
    alloc(w->kind, sizeof(int32_t) * w->Npad);
    alloc(w->lead_blk, sizeof(uint32_t) * LEAD_WORDS);   // (hipMalloc: aligned to 16 bytes and more)
    alloc(w->ep_mem, sizeof(uint32_t) * 8);
    if (w->split) {
        alloc(w->plist, sizeof(int32_t) * (w->maxp <= 16 ? 16 : 32) * w->S);
        alloc(w->plist_cnt, sizeof(int32_t) * w->S);
    }
    for (int k = 0; k < 2; ++k) {
        alloc(w->ids[k], line_bytes(w->H));
        alloc(w->spill[k], spill_bytes);
        if (w->slot_snapshots) alloc(w->pos[k], slot_snapshot_bytes(w));
    }
    alloc(w->err, sizeof(int32_t));
    if (!arc) arc = w->err_host.alloc(sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent);
    if (arc) return bail(arc);
    w->gen = w->lead_blk + LEAD_GEN;
    *w->err_host = 0;
    if (hipStreamCreateWithFlags(&w->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&w->cap_stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(RB_ENODEV, "hipStreamCreate failed"));
    w->stream = w->own_stream;
    {
        const std::pair<void *, size_t> zero[] = {
            {w->snap[0], snap_bytes(w)}, {w->snap[1], snap_bytes(w)}, {w->state, state_bytes(w)},
            // bucket headers of generation 0: every table's generation is >= 2
            {w->ids[0], line_bytes(w->H)}, {w->ids[1], line_bytes(w->H)}, {w->spill[0], spill_bytes}, {w->spill[1], spill_bytes},
            {w->lead_blk, sizeof(uint32_t) * LEAD_WORDS}, {w->ep_mem, sizeof(uint32_t) * 8}, {w->err, sizeof(int32_t)}, {w->defer_cnt, sizeof(int32_t) * 2}};
        for (const auto &z : zero)
            if (z.first && hipMemsetAsync(z.first, 0, z.second, w->stream) != hipSuccess)
                return bail(fail(RB_ENODEV, "hipMemsetAsync failed"));
    }
    std::vector<double> bound;
    int rc = by_real(w->dtype, [&](auto t) { return upload_consts<decltype(t)>(w, d, bound); });
    if (rc) return bail(rc);
    w->bound = std::move(bound);
    *out = w;
    return RB_OK;
}

void rb_world_destroy(rb_world *w) {
    ApiScope api_scope_(w ? w->device : -1);
    if (w) {
        (void)hipSetDevice(w->device);
        (void)hipStreamSynchronize(w->stream);
    }
    free_world(w);
}

int rb_set_stream(rb_world *w, void *s) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w) return fail(RB_EINVAL, "null world");
    HIPCHK(hipSetDevice(w->device));
    // work queued on the old stream (a block run's check included)
    // finishes there before later work is ordered on the new one
    if (int rc = finish_pending(w)) return rc;
    HIPCHK(hipStreamSynchronize(w->stream));
    w->stream = (hipStream_t)s;        // NULL = HIP's null stream
    return RB_OK;
}

int rb_set_xfrc(rb_world *w, const double *xf) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w) return fail(RB_EINVAL, "null world");
    HIPCHK(hipSetDevice(w->device));
    if (int rc = finish_pending(w)) return rc;
    if (!xf) {
        // (graphs capture whether a step reads applied forces)
        if (w->xfrc) { drop_graphs(w); HIPCHK(hipStreamSynchronize(w->stream)); w->xfrc.reset(); }
        return RB_OK;
    }
    if (!w->xfrc) { drop_graphs(w); WCHK(w->xfrc.alloc((size_t)w->esz * 6 * w->S)); }
    HIPCHK(hipStreamSynchronize(w->stream));             // (steps in flight read the old forces)
    return by_real(w->dtype, [&](auto t) {
        using T = decltype(t);
        std::vector<T> h((size_t)6 * w->S, T(0));
        for (int64_t l = 0; l < w->n_local; ++l)
            for (int d = 0; d < 6; ++d) h[(size_t)(d * w->S + l)] = (T)xf[6 * (w->lo + l) + d];
        return wput(w, w->xfrc, h.data(), sizeof(T) * h.size());
    });
}

int rb_record_contacts(rb_world *w, int enable) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w) return fail(RB_EINVAL, "null world");
    HIPCHK(hipSetDevice(w->device));
    if (int rc = finish_pending(w)) return rc;
    if (enable && !w->rec_count) {
        const size_t slots = record_slots(w);
        WCHK(w->rec_count.alloc(sizeof(int32_t) * w->S));
        WCHK(w->rec_partner.alloc(sizeof(int32_t) * slots));
        WCHK(w->rec_kind.alloc(sizeof(int32_t) * slots));
        WCHK(w->rec_dist.alloc((size_t)w->esz * slots));
        WCHK(wfill(w, w->rec_count, 0, sizeof(int32_t) * w->S));
    }
    if (w->record != (enable != 0)) drop_graphs(w);
    w->record = enable != 0;
    return RB_OK;
}

int rb_get_contacts(rb_world *w, int32_t *counts, int32_t *partner, int32_t *kind, double *dist, int64_t cap,
                    int64_t *total) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w || !counts) return fail(RB_EINVAL, "null argument");
    if (!w->rec_count) return fail(RB_EINVAL, "contact recording was never enabled");
    HIPCHK(hipSetDevice(w->device));
    if (int rc = finish_pending(w)) return rc;
    const size_t slots = record_slots(w);
    std::vector<int32_t> c((size_t)w->S), pa(slots), ki(slots);
    std::vector<double> di(slots);
    HIPCHK(hipMemcpyAsync(c.data(), w->rec_count, sizeof(int32_t) * w->S, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipMemcpyAsync(pa.data(), w->rec_partner, sizeof(int32_t) * slots, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipMemcpyAsync(ki.data(), w->rec_kind, sizeof(int32_t) * slots, hipMemcpyDeviceToHost, w->stream));
    WCHK(by_real(w->dtype, [&](auto t) {
        std::vector<decltype(t)> f(slots);
        const int rc = wget(w, f.data(), w->rec_dist, sizeof(f[0]) * slots);
        std::copy(f.begin(), f.end(), di.begin());
        return rc;
    }));
    int64_t t = 0;
    for (int64_t l = 0; l < w->n_local; ++l) {
        const int32_t n = c[(size_t)l] < w->maxrec ? c[(size_t)l] : w->maxrec;
        counts[l] = c[(size_t)l];
        for (int32_t k = 0; k < n; ++k, ++t) {
            if (t < cap) {
                const size_t o = (size_t)l * w->maxrec + k;
                if (partner) partner[t] = pa[o];
                if (kind) kind[t] = ki[o];
                if (dist) dist[t] = di[o];
            }
        }
    }
    if (total) *total = t;
    if (t > cap) return fail(RB_EOVERFLOW, "contact buffer too small: need %lld", (long long)t);
    return RB_OK;
}

int rb_set_contact_law(rb_world *w, int32_t law, double tol) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w) return fail(RB_EINVAL, "null world");
    if (law != RB_LAW_MUJOCO && law != RB_LAW_BALLS) return fail(RB_EINVAL, "unknown contact law %d", law);
    if (!(tol >= 0) || !(tol < 1e6)) return fail(RB_EINVAL, "tol must be finite and >= 0");
    // a law change rebuilds the table from the local snapshot, whose rows of
    // bodies no peer pushed to this rank are stale in halo mode
    if (w->halo) return fail(RB_EUNSUPPORTED, "rb_set_contact_law on a halo-exchanging shard");
    if (law == RB_LAW_BALLS) {
        if (!w->all_spheres) return fail(RB_EUNSUPPORTED, "the two-ball law takes spheres only");
        if (w->P != 1) return fail(RB_EUNSUPPORTED, "the two-ball law steps unsharded worlds only");
        const double ground[6] = {0, 0, 1, 0, 0, 0};
        if (w->n_planes > 1 || (w->n_planes == 1 && memcmp(w->planes[0], ground, sizeof(ground)) != 0))
            return fail(RB_EUNSUPPORTED, "the two-ball law's only plane is the z = 0 ground (ball_collision.py:88-90)");
    }
    HIPCHK(hipSetDevice(w->device));
    if (int rc = finish_pending(w)) return rc;
    HIPCHK(hipStreamSynchronize(w->stream));
    if (law == RB_LAW_BALLS && !w->vel[0]) {
        const size_t bytes = (size_t)w->esz * 8 * w->Npad;
        for (int k = 0; k < 2; ++k) {
            WCHK(w->vel[k].alloc(bytes));
            WCHK(wfill(w, w->vel[k], 0, bytes));
        }
    }
    if (w->law != law) {
        // the default law keeps positions in the snapshot: restore them
        // from the true positions before the snapshot is read again; the
        // other way, the true positions from the snapshot
        const bool to_snap = law == RB_LAW_MUJOCO;
        const size_t esz = (size_t)w->esz;
        std::vector<char> st(state_bytes(w)), sn(snap_bytes(w));
        HIPCHK(hipMemcpyAsync(st.data(), w->state, st.size(), hipMemcpyDeviceToHost, w->stream));
        WCHK(wget(w, sn.data(), w->snap[w->sp()], sn.size()));
        for (int64_t l = 0; l < w->n_local; ++l)
            for (int d = 0; d < 3; ++d) {
                char *in_sn = &sn[esz * (4 * (w->lo + l) + d)], *in_st = &st[esz * ((10 + d) * w->S + l)];
                memcpy(to_snap ? in_sn : in_st, to_snap ? in_st : in_sn, esz);
            }
        WCHK(to_snap ? wput(w, w->snap[w->sp()], sn.data(), sn.size()) : wput(w, w->state, st.data(), st.size()));
    }
    w->law = law;
    w->tol = tol;
    w->state_version += 1;
    w->tile_valid_sp = -1;
    // cell = 2 x the largest reach: 2 x 2 rmax, or 2 x (2 rmax + tol)
    const double reach = law == RB_LAW_BALLS ? 2.0 * w->rmax + tol : 2.0 * w->rmax;
    w->inv_cs = 1.0 / (reach > 0 ? 2.0 * reach * 1.001 : 1.0);
    drop_graphs(w);
    w->primed = false;
    return RB_OK;
}

int rb_world_stats(rb_world *w, int64_t *out, int32_t n) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w || (n > 0 && !out)) return fail(RB_EINVAL, "null argument");
    HIPCHK(hipSetDevice(w->device));
    if (int rc = finish_pending(w)) return rc;
    const bool tile = tile_eligible(w);
    const int form = tile ? FORM_TILE : step_form(w);
    // the epoch counters are advanced by the step kernels: read once the
    // world's work so far is done (only worlds that can have epochs wait)
    unsigned long long ep_count[2] = {0, 0};
    if (n > RB_STAT_APPEND_STEPS && epoch_eligible(w)) WCHK(wget(w, ep_count, w->ep_mem + 4, sizeof(ep_count)));
    const int64_t v[RB_STATS_COUNT] = {(int64_t)w->graphs.size(), form, w->box_stats[0], w->box_stats[1], w->refits,
                                       w->table_grows, w->H, (int64_t)w->maxp, w->io_stats[0], w->io_stats[1],
                                       w->tile_stats[0], w->tile_stats[1], w->tile_stats[2], w->tile_stats[3],
                                       (int64_t)w->tile_why_seen, (int64_t)w->tile_ntx * w->tile_nty,
                                       (int64_t)w->tile_tc, tile && w->tile_skip == 0 ? 1 : 0, step_form(w),
                                       (int64_t)ep_count[0], (int64_t)ep_count[1], (int64_t)w->epoch_max,
                                       (int64_t)(uint32_t)w->group,
                                       step_form(w) == FORM_WIDE_HELP && w->help_search ? 1 : 0};
    for (int32_t k = 0; k < n && k < RB_STATS_COUNT; ++k) out[k] = v[k];
    return n < RB_STATS_COUNT ? n : RB_STATS_COUNT;
}

int rb_query(rb_world *w, int64_t *n_owned, int64_t *bytes) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w) return fail(RB_EINVAL, "null world");
    if (n_owned) *n_owned = w->n_local;
    if (bytes) *bytes = w->bytes_per_body_step;
    return RB_OK;
}

int rb_tile_config(rb_world *w, int32_t mode, int32_t kmax, double band, int64_t owned) {
    ApiScope api_scope_(w ? w->device : -1);
    (void)kmax;
    (void)band;
    (void)owned;
    if (!w) return fail(RB_EINVAL, "null world");
    if (mode == -1 || mode == 0) return RB_OK;
    if (mode == 1) return fail(RB_EUNSUPPORTED, "rb_tile_config: the tile blocks were retired (librbhip 0.3)");
    return fail(RB_EINVAL, "rb_tile_config: mode must be -1, 0 or 1");
}

int rb_kernel_timing(rb_world *w, int enable, double *avg_ms, int64_t *launches) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w) return fail(RB_EINVAL, "null world");
    HIPCHK(hipSetDevice(w->device));
    int rc = collect_timing(w);
    if (rc) return rc;
    if (avg_ms) *avg_ms = w->t_n ? w->t_sum_ms / (double)w->t_n : 0.0;
    if (launches) *launches = w->t_n;
    if (enable && !w->timing) { w->t_sum_ms = 0; w->t_n = 0; }
    w->timing = enable != 0;
    return RB_OK;
}

}  // extern "C"
