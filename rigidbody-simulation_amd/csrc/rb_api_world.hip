// rb_api_world.hip — a world's lifetime (rb_world_create with its environment
// switches, the constants' upload, rb_world_destroy), its small setters and
// its queries.
#include <array>

#include "rb_host.hpp"

using namespace rb::host;

namespace {

int64_t next_pow2(int64_t v) {
    int64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

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
            HIPCHK(hipMalloc((void **)&w->tile_type_of, (size_t)w->N));
            WCHK(wput(w, w->tile_type_of, type_of.data(), (size_t)w->N));
            w->tile_ntypes = (int32_t)types.size();
        }
    }
    std::vector<int32_t> k((size_t)w->Npad, 0);
    for (int64_t b = 0; b < w->N; ++b) k[(size_t)b] = d->kind[b];
    WCHK(wput(w, w->kind, k.data(), sizeof(int32_t) * k.size()));
    return RB_OK;
}

void free_world(rb_world *w) {
    if (!w) return;
    (void)hipSetDevice(w->device);
    drop_graphs(w);
    shard_release(w);
    for (auto &pr : w->tev) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    if (w->opt_save) (void)hipFree(w->opt_save);
    void *tbufs[] = {w->tile_mem, w->tile_fill, w->tile_gen, w->tile_why, w->tile_commits, w->tile_type_of};
    for (void *b : tbufs)
        if (b) (void)hipFree(b);
    if (w->tile_host) (void)hipHostFree(w->tile_host);
    if (w->tile_pub_host) (void)hipHostFree(w->tile_pub_host);
    if (w->defer_host) (void)hipHostFree(w->defer_host);
    if (w->io_q_h) (void)hipHostFree(w->io_q_h);
    if (w->io_v_h) (void)hipHostFree(w->io_v_h);
    if (w->io_q_d) (void)hipFree(w->io_q_d);
    if (w->io_v_d) (void)hipFree(w->io_v_d);
    for (hipEvent_t &e : w->io_ev)
        if (e) (void)hipEventDestroy(e);
    void *bufs[] = {w->snap[0], w->snap[1], w->qsnap[0], w->qsnap[1], w->defer_q, w->defer_cnt, w->state, w->consts, w->kind, w->xfrc, w->lead_blk, w->ep_mem,
                    w->ids[0], w->ids[1], w->spill[0], w->spill[1], w->pos[0], w->pos[1], w->plist, w->plist_cnt, w->vel[0], w->vel[1], w->err, w->rec_count, w->rec_partner, w->rec_kind,
                    w->rec_dist, w->cq_line, w->cq_spill, w->cq_words, w->cq_stage};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    if (w->err_host) (void)hipHostFree(w->err_host);
    if (w->cq_stage_h) (void)hipHostFree(w->cq_stage_h);
    if (w->own_stream) (void)hipStreamDestroy(w->own_stream);
    if (w->cap_stream) (void)hipStreamDestroy(w->cap_stream);
    delete w;
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

    rb_world *w = new rb_world();
    w->dtype = d->dtype;
    w->esz = d->dtype == RB_F64 ? 8 : 4;
    w->device = d->device;
    w->N = d->n_bodies;
    w->P = d->world_size;
    w->rank = d->rank;
    w->S = (w->N + w->P - 1) / w->P;
    w->Npad = w->S * w->P;
    w->lo = w->S * w->rank;
    const int64_t hi = w->lo + w->S < w->N ? w->lo + w->S : w->N;
    w->n_local = (int32_t)(hi > w->lo ? hi - w->lo : 0);
    w->n_planes = d->n_planes;
    for (int k = 0; k < d->n_planes; ++k)
        for (int j = 0; j < 6; ++j) w->planes[k][j] = d->planes[6 * k + j];
    for (int j = 0; j < 3; ++j) w->g[j] = d->gravity[j];
    w->oriented = d->normal_convention == RB_NORMAL_ORIENTED;
    w->maxp = maxp;
    bool any_box = false;
    for (int64_t b = 0; b < d->n_bodies && !any_box; ++b) any_box = d->kind[b] != RB_BODY_SPHERE;
    // box-capable kernels (sharded worlds exchange the boxes' orientations)
    w->boxes = any_box;
    // records per body: 4 per plane, 1 per sphere partner, up to 4 per
    // partner in scenes with boxes (oracle/rb_oracle_impl.h contact_stride)
    w->maxrec = 4 * w->n_planes + (any_box ? 4 : 1) * w->maxp;
    // worlds with boxes: the cooperative form only up to 4,608 owned bodies
    // (cubes on the incline, per step, helper / plain cooperative / wide:
    // 4,096 8.6 / 10.7 / 11.7 us, 5,184 10.4 / 12.4 / 10.2, 9,216 12.9 /
    // 15.7 / 10.2, 16,384 14.7 (plain) / 12.2; scripts/form_ab.py)
    if (any_box) w->coop_max = 4608;
    // worlds with boxes keep the helper wave without a share of the search
    // (C5, 16,384 cubes: about 20 % slower per step with it;
    // profiles/help_search/shapes_ab.log)
    if (any_box) w->help_search = false;
    if (const char *ev = getenv("RBHIP_COOP_MAX_BODIES")) w->coop_max = atoll(ev);
    if (const char *ev = getenv("RBHIP_WIDE_MAX_BODIES")) w->wide_max = atoll(ev);
    if (const char *ev = getenv("RBHIP_HELP_MAX_BODIES")) w->help_max = atoll(ev);
    if (const char *ev = getenv("RBHIP_WIDE_HELP")) w->wide_help = atoi(ev) != 0;
    if (const char *ev = getenv("RBHIP_HELP_SEARCH")) w->help_search = atoi(ev) != 0;
    // the cell-ordered tile form (rb_tiles.hip): RBHIP_TILE = 0 off, 1 every
    // eligible world, -1 auto, the default (eligible worlds of >=
    // RBHIP_TILE_MIN_BODIES bodies, until their first roll-back): it measures
    // slower than the hashed forms up to 65,536 flat spheres (C3) and faster
    // from 73,984 up
    if (const char *ev = getenv("RBHIP_TILE")) w->tile_mode = atoi(ev) < 0 ? -1 : atoi(ev) ? 1 : 0;
    w->tile_mode_init = w->tile_mode;
    if (const char *ev = getenv("RBHIP_TILE_MIN_BODIES")) w->tile_min_bodies = atoll(ev);
    if (const char *ev = getenv("RBHIP_BOX_OPTIMISTIC")) w->box_opt = atoi(ev) != 0;
    if (const char *ev = getenv("RBHIP_DIAG_OVERFLOW")) w->diag_overflow = atoi(ev);
    if (const char *ev = getenv("RBHIP_TABLE_EPOCH")) w->epoch_max = std::max(1, std::min(EPOCH_MAX, atoi(ev)));
    // rb_query_contacts: the bound of its staging buffer
    if (const char *ev = getenv("RBHIP_CONTACT_STAGE_BYTES"))
        if (atoll(ev) > 0) w->cq_limit = (size_t)atoll(ev);
    // buckets: cooperative worlds (a hash per cell; they also keep a slot
    // snapshot line per bucket) 16 per body; the one-lane and wide forms
    // (linear cell groups, below) 32 per body, so the groups' period spans
    // the scene (C3: 2^21 buckets, 205 m x 102 m x 12.8 m; as fast as 2^23,
    // 16 per body 20 % slower: the period then folds the scene onto itself).
    // At most 2^26 buckets (8 GB of lines per table).
    const bool coop_world = w->n_local <= w->coop_max;
    int64_t want = coop_world ? 16 * w->N : 32 * w->N;
    if (const char *ev = getenv("RBHIP_HASH_FACTOR"))
        if (atoll(ev) > 0) want = atoll(ev) * w->N;
    if (want < 4096) want = 4096;
    // memory cap over both tables (lines, plus slot snapshots in cooperative
    // worlds): RBHIP_HASH_MAX_BYTES, default 8 GiB (1M bodies keep 32 buckets
    // per body, 4M bodies get 8)
    const int64_t per_bucket = 2 * (int64_t)(sizeof(uint32_t) * LINE_WORDS + (coop_world ? w->esz * 4 * LINE_WORDS : 0));
    int64_t cap_bytes = int64_t(8) << 30;
    if (const char *ev = getenv("RBHIP_HASH_MAX_BYTES"))
        if (atoll(ev) > 0) cap_bytes = atoll(ev);
    int64_t hmax = 4096;
    while (hmax * 2 * per_bucket <= cap_bytes && hmax < (int64_t(1) << 26)) hmax *= 2;
    w->H = next_pow2(want) < hmax ? next_pow2(want) : hmax;
    w->hmax = hmax;
    // The one-lane and wide forms group cells 8x8x4, the buckets of a group
    // contiguous (32 KB of lines), and lay the groups out linearly, periodic
    // in 2^lx x 2^ly x 2^lz groups (below): against a hash per cell measured
    // 6 % faster at 65k bodies (flat), 5 % (incline), 12 % at 1M; hashed
    // groups were bimodal (a group collision doubles the bodies of every
    // bucket in both groups and sends waves through the wide form's extra
    // round trip for buckets of 7+ ids).  Those kernels compute
    // the linear layout directly (rb_grid.hpp LAYOUT_LINEAR), so their worlds
    // always use it.  The cooperative form keeps a hash per cell.
    // RBHIP_HASH_GROUP=bx:by:bz sets the group shape (2^bx x 2^by x 2^bz
    // cells); in cooperative worlds bx:by:bz hashes the groups and
    // bx:by:bz:l lays them out linearly.
    int gshape = coop_world ? 0 : 0x233;
    bool linear = !coop_world;
    if (const char *ev = getenv("RBHIP_HASH_GROUP")) {
        int bx = 0, by = 0, bz = 0;
        char mode = 'h';
        if (sscanf(ev, "%d:%d:%d:%c", &bx, &by, &bz, &mode) >= 3 && bx >= 0 && by >= 0 && bz >= 0 && bx + by + bz <= 12)
            gshape = bx | (by << 4) | (bz << 8);
        if (coop_world) linear = mode == 'l';
    }
    auto gbits = [](int g) { return (g & 15) + ((g >> 4) & 15) + ((g >> 8) & 15); };
    // a table too small for the groups: smaller groups (linear), none (hashed)
    while (gshape && (int64_t(1) << gbits(gshape)) > w->H / 4) {
        if (!linear) { gshape = 0; break; }
        for (int sh = 8; sh >= 0; sh -= 4)
            if ((gshape >> sh) & 15) { gshape -= 1 << sh; break; }
    }
    w->group = gshape;
    if (linear) {
        // the group slots split into a period of 2^lx x 2^ly x 2^lz groups (z: at most 8)
        int lg = 0;
        while ((int64_t(1) << (lg + 1)) <= w->H) ++lg;
        lg -= gbits(gshape);
        const int lz = lg / 3 < 3 ? lg / 3 : 3, lx = (lg - lz + 1) / 2, ly = lg - lz - lx;
        int l[3] = {lx, ly, lz};
        // diagnostic: RBHIP_HASH_PERIOD=lx:ly:lz sets the creation-time split
        // (at most the table's group bits; with RBHIP_FIT_PERIOD=0 it stays).
        // A zero on an axis whose groups are one cell thick makes a body's
        // two cells along that axis one bucket (tests of the visit-once rule)
        if (const char *ev = getenv("RBHIP_HASH_PERIOD")) {
            int a = 0, b = 0, c = 0;
            if (sscanf(ev, "%d:%d:%d", &a, &b, &c) == 3 && a >= 0 && b >= 0 && c >= 0 && a <= 15 && b <= 15 && c <= 15 &&
                a + b + c <= lg) { l[0] = a; l[1] = b; l[2] = c; }
        }
        w->group |= (l[0] << 12) | (l[1] << 16) | (l[2] << 20) | (1 << 24);
    }
    // heads per 128-byte line (rb_internal.hpp Table): 4 in wide-form worlds
    // (C3 17.4 -> 16.4 us), 2 in one-lane worlds (1M 0.237 -> 0.225 ms; 4
    // there cost 10 % at 262k), 1 in cooperative worlds (no gain measured).
    // The cooperative and wide kernels assume theirs at compile time;
    // RBHIP_HEADS_PER_LINE = 1, 2 or 4 sets the one-lane worlds'.
    const bool wide_world = !coop_world && w->n_local <= w->wide_max;
    int rl = coop_world ? 0 : wide_world ? 2 : 1;
    if (const char *ev = getenv("RBHIP_HEADS_PER_LINE"))
        if (!coop_world && !wide_world) {
            const int r = atoi(ev);
            if (r == 1 || r == 2 || r == 4) rl = r == 1 ? 0 : r == 2 ? 1 : 2;
        }
    w->group |= rl << 25;
    int64_t nsph = 0;
    for (int64_t b = 0; b < w->N; ++b) nsph += d->kind[b] == RB_BODY_SPHERE;
    // algorithmic bytes per body-step: 13 state reals read + 13
    // written + constants (m, I[3], r | h[3])
    w->bytes_per_body_step = (int64_t)w->esz * (26 + 4) + (int64_t)w->esz * ((nsph * 1 + (w->N - nsph) * 3) / w->N);

    auto bail = [&](int rc) { free_world(w); return rc; };
    if (hipSetDevice(w->device) != hipSuccess) return bail(fail(RB_ENODEV, "hipSetDevice(%d) failed", w->device));
#define ALLOC(ptr, bytes)                                                                        \
    do {                                                                                         \
        if (hipMalloc((void **)&(ptr), (bytes)) != hipSuccess)                                   \
            return bail(fail(RB_ENOMEM, "hipMalloc(%lld) failed", (long long)(bytes)));          \
    } while (0)
    for (int k = 0; k < 2; ++k) ALLOC(w->snap[k], (size_t)w->esz * 4 * w->Npad);
    if (w->boxes) {
        for (int k = 0; k < 2; ++k) ALLOC(w->qsnap[k], (size_t)w->esz * 4 * w->Npad);
        ALLOC(w->defer_q, sizeof(int32_t) * (w->S > 0 ? w->S : 1));
        ALLOC(w->defer_cnt, sizeof(int32_t) * 2);
    }
    ALLOC(w->state, (size_t)w->esz * 13 * w->S);
    ALLOC(w->consts, (size_t)w->esz * 8 * w->Npad);
    ALLOC(w->kind, sizeof(int32_t) * w->Npad);
    ALLOC(w->lead_blk, sizeof(uint32_t) * LEAD_WORDS);   // (hipMalloc: aligned to 16 bytes and more)
    w->gen = w->lead_blk + LEAD_GEN;
    ALLOC(w->ep_mem, sizeof(uint32_t) * 8);
    // Opt-in (RBHIP_SPLIT=1): large scenes step in two kernels (search,
    // update) joined by a partner list; bit-exact with the oracle on the
    // device (tests/test_gpu_parity.py ragged-scene test) but no faster
    // (DESIGN §5), so the default is the fused one-kernel step.
    const char *split_env = getenv("RBHIP_SPLIT");
    const bool coop = w->n_local <= w->coop_max;
    const bool split = !coop && !w->boxes && split_env && atoi(split_env) == 1;
    if (split) {
        ALLOC(w->plist, sizeof(int32_t) * (w->maxp <= 16 ? 16 : 32) * w->S);
        ALLOC(w->plist_cnt, sizeof(int32_t) * w->S);
    }
    for (int k = 0; k < 2; ++k) {
        ALLOC(w->ids[k], sizeof(uint32_t) * LINE_WORDS * w->H);
        ALLOC(w->spill[k], sizeof(uint32_t) * SPILL_LINE_WORDS * SPILL_LINES);
        // slot snapshots feed the cooperative search only
        if (needs_slot_snapshots(coop, split)) ALLOC(w->pos[k], (size_t)w->esz * 4 * LINE_WORDS * w->H);
    }
    ALLOC(w->err, sizeof(int32_t));
#undef ALLOC
    if (hipHostMalloc((void **)&w->err_host, sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void **)&w->err_host_d, w->err_host, 0) != hipSuccess)
        return bail(fail(RB_ENOMEM, "hipHostMalloc failed"));
    *w->err_host = 0;
    if (hipStreamCreateWithFlags(&w->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&w->cap_stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(RB_ENODEV, "hipStreamCreate failed"));
    w->stream = w->own_stream;
    {
        const std::pair<void *, size_t> zero[] = {
            {w->snap[0], (size_t)w->esz * 4 * w->Npad}, {w->snap[1], (size_t)w->esz * 4 * w->Npad},
            {w->state, (size_t)w->esz * 13 * w->S},
            // bucket headers of generation 0: every table's generation is >= 2
            {w->ids[0], sizeof(uint32_t) * LINE_WORDS * w->H}, {w->ids[1], sizeof(uint32_t) * LINE_WORDS * w->H},
            {w->spill[0], sizeof(uint32_t) * SPILL_LINE_WORDS * SPILL_LINES},
            {w->spill[1], sizeof(uint32_t) * SPILL_LINE_WORDS * SPILL_LINES},
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
        if (w->xfrc) { drop_graphs(w); HIPCHK(hipStreamSynchronize(w->stream)); HIPCHK(hipFree(w->xfrc)); w->xfrc = nullptr; }
        return RB_OK;
    }
    if (!w->xfrc) { drop_graphs(w); HIPCHK(hipMalloc(&w->xfrc, (size_t)w->esz * 6 * w->S)); }
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
        const size_t slots = (size_t)w->maxrec * (w->S > 0 ? w->S : 1);
        HIPCHK(hipMalloc((void **)&w->rec_count, sizeof(int32_t) * w->S));
        HIPCHK(hipMalloc((void **)&w->rec_partner, sizeof(int32_t) * slots));
        HIPCHK(hipMalloc((void **)&w->rec_kind, sizeof(int32_t) * slots));
        HIPCHK(hipMalloc(&w->rec_dist, (size_t)w->esz * slots));
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
    const size_t slots = (size_t)w->maxrec * w->S;
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
            if (hipMalloc(&w->vel[k], bytes) != hipSuccess) return fail(RB_ENOMEM, "hipMalloc(%zu) failed", bytes);
            WCHK(wfill(w, w->vel[k], 0, bytes));
        }
    }
    if (w->law != law) {
        // the default law keeps positions in the snapshot: restore them
        // from the true positions before the snapshot is read again; the
        // other way, the true positions from the snapshot
        const bool to_snap = law == RB_LAW_MUJOCO;
        const size_t esz = (size_t)w->esz;
        std::vector<char> st(esz * 13 * w->S), sn(esz * 4 * w->Npad);
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
