// rb_api_contacts.hip — the queries of a world's current state: the contact
// query, rb_query_contacts (host arrays, synchronous) and rb_query_contacts_dev
// (device arrays, enqueued), and the impulse query of the next step,
// rb_query_impulses and rb_query_impulses_dev, alike.
// Kernels: rb_world_contacts.hip, rb_world_impulses.hip, and the insert kernel
// of rb_io.hip.
//
// The two queries share one broadphase table, one staging buffer and one way
// through a call.  The table (bucket lines, spill lines, a generation word and
// an error word) is the queries' own: allocated at the first query, freed with
// the world.
// Every call bumps the table's generation, inserts every body of the current
// snapshot into it and runs the query kernel over it.  It uses the world's
// grid (cell size, bucket count, layout) as it stands at the call, and never
// the tables the steps use: after rb_set_state those are stale, and inside an
// append epoch they are not a plain table.  Nothing here changes a field of
// the world that a step, a graph, the stats or the boundary reads: the fields
// written are the cq_* ones alone.
#include <cmath>

#include "rb_host.hpp"
#include "rb_stagelayout.hpp"
#include "rb_world_contacts.hpp"
#include "rb_world_impulses.hpp"

namespace rb::host {

// the arguments both forms share, before any device call
static int query_check(const rb_world *w, int64_t first, int64_t count, int32_t R, const void *counts, const void *partner,
                       const void *kind, const void *dist, const void *pos, const void *frame) {
    if (!w) return fail(RB_EINVAL, "null world");
    if (!counts) return fail(RB_EINVAL, "counts NULL");
    if (R < 0) return fail(RB_EINVAL, "max_records < 0");
    const int given = (partner != nullptr) + (kind != nullptr) + (dist != nullptr);
    if (given != 0 && given != 3) return fail(RB_EINVAL, "partner, kind and dist may be NULL only all together");
    if (R == 0 && (given || pos || frame)) return fail(RB_EINVAL, "max_records 0 with record arrays given");
    if (R > 0 && !given)
        return fail(RB_EINVAL, "max_records %d with partner, kind and dist NULL (a counts-only query has max_records 0)", R);
    if (first < 0 || count < 0 || first > w->N || count > w->N - first)
        return fail(RB_EINVAL, "bodies [%lld, %lld + %lld) outside [0, %lld)", (long long)first, (long long)first,
                    (long long)count, (long long)w->N);
    return RB_OK;
}
// the impulse query's: the contact query's (jn and jt with the records), rb_step's parameters, finite
static int impulse_check(const rb_world *w, int64_t first, int64_t count, int32_t R, const void *counts, const void *partner,
                         const void *kind, const void *dist, const void *jn, const void *jt, double dt, double e, double mu,
                         double thr) {
    WCHK(query_check(w, first, count, R, counts, partner, kind, dist, nullptr, nullptr));
    if ((jn != nullptr) != (partner != nullptr) || (jt != nullptr) != (partner != nullptr))
        return fail(RB_EINVAL, "partner, kind, dist, jn and jt may be NULL only all together (max_records 0)");
    if (!(dt > 0) || !(e >= 0) || !(mu >= 0) || !(thr >= 0))
        return fail(RB_EINVAL, "invalid step parameters dt=%g e=%g mu=%g thr=%g", dt, e, mu, thr);
    if (!std::isfinite(dt) || !std::isfinite(e) || !std::isfinite(mu) || !std::isfinite(thr))
        return fail(RB_EINVAL, "non-finite step parameters dt=%g e=%g mu=%g thr=%g", dt, e, mu, thr);
    return RB_OK;
}
static int query_supported(const rb_world *w) {
    if (w->P > 1) return fail(RB_EUNSUPPORTED, "the contact and impulse queries are for world_size 1");
    if (w->law == RB_LAW_BALLS)
        return fail(RB_EUNSUPPORTED, "the two-ball law has no contact list (its hit test carries a tolerance of its own)");
    return RB_OK;
}

// The query's table for the world's grid as it stands.  A table of another
// size or line layout is dropped (table growth): headers of the old layout
// would be read as ids, and ids as headers.  (The layout word without the
// period's split, layout_key: refits move the split only, and what is left
// decides where a bucket's header lies in the lines.)
static int query_table(rb_world *w) {
    const size_t lines = line_bytes(w->H), spill = spill_bytes;
    if (w->cq_line && (w->cq_H != w->H || w->cq_layout != layout_key(w->group))) {
        HIPCHK(hipStreamSynchronize(w->stream));     // (a query in flight reads it)
        w->cq_line.reset();
    }
    if (!w->cq_line) {
        WCHK(w->cq_line.alloc(lines));
        w->cq_H = w->H;
        w->cq_layout = layout_key(w->group);
        w->cq_gen = 0;
    }
    if (!w->cq_spill) WCHK(w->cq_spill.alloc(spill));
    if (!w->cq_words) WCHK(w->cq_words.alloc(sizeof(uint32_t) * 2));
    // headers of generation 0 are empty buckets: a new table, and one whose
    // generations are used up, starts from zeros
    if (w->cq_gen == 0 || w->cq_gen == UINT32_MAX) {
        HIPCHK(hipMemsetAsync(w->cq_line, 0, lines, w->stream));
        HIPCHK(hipMemsetAsync(w->cq_spill, 0, spill, w->stream));
        w->cq_gen = 0;
    }
    return RB_OK;
}

// what the kernels of one call read: sp.cur is the query's table
template <typename T> static WorldContactQuery<T> make_query(const rb_world *w) {
    WorldContactQuery<T> q{};
    StepParams<T> &p = q.sp;
    p.snap_cur = dp<Snap<T>>(w->snap[w->sp()], 0);
    p.st = BodyState<T>{dp<T>(w->state, 0), w->S};
    p.cs = BodyConsts<T>{dp<T>(w->consts, 0), w->Npad, w->kind};
    p.n_local = w->n_local;
    p.n_global = w->N;
    p.S = (int32_t)w->S;
    p.n_planes = w->n_planes;
    for (int k = 0; k < w->n_planes; ++k)
        for (int d = 0; d < 3; ++d) { p.pn[k][d] = (T)w->planes[k][d]; p.pp[k][d] = (T)w->planes[k][3 + d]; }
    p.grid.inv_cs = (T)w->inv_cs;
    p.grid.hmask = (uint32_t)(w->H - 1);
    p.grid.H = (int32_t)w->H;
    p.grid.super = w->group;
    p.cur = Table<T>{w->cq_line, nullptr, w->cq_words, w->cq_spill};
    p.err = reinterpret_cast<int32_t *>(w->cq_words + 1);
    return q;
}

// the impulse query's block: beside the above, what the solve of a step reads, as make_step fills it
template <typename T> static WorldImpulseQuery<T> make_impulse_query(const rb_world *w, double dt, double e, double mu, double thr) {
    WorldImpulseQuery<T> q{};
    q.c = make_query<T>(w);
    StepParams<T> &p = q.c.sp;
    p.xfrc = w->xfrc ? dp<T>(w->xfrc, 0) : nullptr;
    for (int d = 0; d < 3; ++d) p.g[d] = (T)w->g[d];
    p.dt = (T)dt; p.e = (T)e; p.mu = (T)mu; p.thr = (T)thr;
    p.oriented = w->oriented;
    return q;
}

// a call's first part: the next generation, a clean error word, every body
// of the current snapshot into the table
static int query_fill(rb_world *w) {
    WCHK(query_table(w));
    w->cq_gen += 1;
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)w->cq_words, (int)w->cq_gen, 1, w->stream));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(w->cq_words + 1), 0, 1, w->stream));
    HIPCHK(by_real(w->dtype, [&](auto t) {
        using T = decltype(t);
        const WorldContactQuery<T> q = make_query<T>(w);
        InsertParams<T> ip{};
        ip.snap = q.sp.snap_cur;
        ip.kind = w->kind;
        ip.first = 0;
        ip.count = w->N;
        ip.grid = q.sp.grid;
        ip.tab = q.sp.cur;
        ip.err = q.sp.err;
        return launch_insert<T>(ip, w->stream);
    }));
    return RB_OK;
}

// bodies [first, first + count) into the given arrays (device memory)
static int query_launch(rb_world *w, int64_t first, int64_t count, int32_t R, int32_t *counts, int32_t *partner,
                        int32_t *kind, void *dist, void *pos, void *frame, bool io32) {
    HIPCHK(by_real(w->dtype, [&](auto t) {
        using T = decltype(t);
        WorldContactQuery<T> q = make_query<T>(w);
        q.counts = counts; q.partner = partner; q.kind = kind;
        q.dist = dist; q.pos = pos; q.frame = frame;
        q.first = first; q.count = count;
        q.R = R;
        q.io32 = io32;
        return launch_world_contacts<T>(q, w->boxes, w->stream);
    }));
    return RB_OK;
}

// The staging of the host form: a device buffer and its pinned twin, grown
// on demand up to the world's bound (laid out by rb_stagelayout.hpp, a body
// per unit).  cq_stage_bytes counts once both stand.
static int stage_reserve(rb_world *w, size_t bytes) {
    if (bytes <= w->cq_stage_bytes) return RB_OK;
    HIPCHK(hipStreamSynchronize(w->stream));
    w->cq_stage_bytes = 0;
    WCHK(w->cq_stage.alloc(bytes));
    WCHK(w->cq_stage_h.alloc(bytes, hipHostMallocDefault));
    w->cq_stage_bytes = bytes;
    return RB_OK;
}

// The host form of either query: the ranges of bodies that fit the staging
// buffer, one launch each (launch(first body, bodies, staging base)), one DMA
// per array into the pinned twin, then out to the caller's arrays dst (in the
// layout's field order).
template <typename Launch>
static int staged_ranges(rb_world *w, const StageLayout &lay, const char *what, int64_t first, int64_t count, void *const *dst,
                         Launch launch) {
    const size_t per = lay.per();
    if (per > w->cq_limit)
        return fail(RB_EINVAL, "%s of one body (%zu bytes) does not fit the staging buffer (%zu bytes: "
                               "RBHIP_CONTACT_STAGE_BYTES)", what, per, w->cq_limit);
    const int64_t fit = std::min<int64_t>(count, lay.fit(w->cq_limit));
    HIPCHK(hipSetDevice(w->device));
    if (int rc = finish_pending(w)) return rc;
    WCHK(stage_reserve(w, per * (size_t)fit));
    WCHK(query_fill(w));
    for (int64_t at0 = 0; at0 < count; at0 += fit) {
        const size_t c = (size_t)std::min<int64_t>(fit, count - at0);
        char *d = w->cq_stage, *h = w->cq_stage_h;
        WCHK(launch(first + at0, c, d));
        for (int f = 0; f < lay.n; ++f)
            if (lay.unit[f])
                HIPCHK(hipMemcpyAsync(h + lay.offset(f, c), d + lay.offset(f, c), lay.bytes(f, c), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(hipStreamSynchronize(w->stream));     // (the next sub-range reuses the staging)
        for (int f = 0; f < lay.n; ++f)
            if (lay.unit[f]) memcpy((char *)dst[f] + lay.caller(f, (size_t)at0), h + lay.offset(f, c), lay.bytes(f, c));
    }
    return RB_OK;
}

// what a host form returns: the reason of the first body without a list, if any
static int list_status(rb_world *w, const char *what, const int32_t *counts, int64_t first, int64_t count) {
    const int64_t bad = std::find(counts, counts + count, QUERY_NO_LIST) - counts;
    if (bad == count) return RB_OK;
    int32_t bits = 0;
    WCHK(wget(w, &bits, w->cq_words + 1, sizeof bits));
    if (bits & ERR_BUCKET_OVERFLOW)
        return fail(RB_EOVERFLOW, "%s: its broadphase table overflowed; no body has a list (first: body %lld)", what,
                    (long long)(first + bad));
    if (bits & ERR_PARTNER_OVERFLOW)
        return fail(RB_EOVERFLOW, "%s: body %lld has more than %d partners in reach (or no valid position): no list", what,
                    (long long)(first + bad), QUERY_MAXP);
    return fail(RB_EDOM, "%s: body %lld has a non-finite or out-of-range position: no list", what, (long long)(first + bad));
}

// bodies [first, first + count) of the impulse query into the given arrays (device memory)
static int impulse_launch(rb_world *w, int64_t first, int64_t count, int32_t R, double dt, double e, double mu, double thr,
                          int32_t *counts, int32_t *partner, int32_t *kind, void *dist, void *jn, void *jt, void *vel,
                          void *net, bool io32) {
    HIPCHK(by_real(w->dtype, [&](auto t) {
        using T = decltype(t);
        WorldImpulseQuery<T> q = make_impulse_query<T>(w, dt, e, mu, thr);
        q.c.counts = counts; q.c.partner = partner; q.c.kind = kind; q.c.dist = dist;
        q.c.first = first; q.c.count = count;
        q.c.R = R;
        q.c.io32 = io32;
        q.jn = jn; q.jt = jt; q.vel = vel; q.net = net;
        return launch_world_impulses<T>(q, w->boxes, w->stream);
    }));
    return RB_OK;
}

}  // namespace rb::host

using namespace rb::host;

extern "C" {

int rb_query_contacts(rb_world *w, int64_t first, int64_t count, int32_t max_records, int32_t *counts, int32_t *partner,
                      int32_t *kind, double *dist, double *pos, double *frame, int64_t *n_truncated) {
    ApiScope api_scope_(w ? w->device : -1);
    const int32_t R = max_records;
    WCHK(query_check(w, first, count, R, counts, partner, kind, dist, pos, frame));
    WCHK(query_supported(w));
    if (n_truncated) *n_truncated = 0;
    if (count == 0) return RB_OK;
    const StageLayout lay = stage_contacts(1, R, pos, frame);
    void *const dst[SC_FIELDS] = {dist, pos, frame, counts, partner, kind};
    WCHK(staged_ranges(w, lay, "the contact list", first, count, dst, [&](int64_t at, size_t c, char *d) {
        return query_launch(w, at, (int64_t)c, R, (int32_t *)lay.at(d, SC_COUNTS, c), (int32_t *)lay.at(d, SC_PARTNER, c),
                            (int32_t *)lay.at(d, SC_KIND, c), lay.at(d, SC_DIST, c), lay.at(d, SC_POS, c), lay.at(d, SC_FRAME, c),
                            false);
    }));
    if (n_truncated) *n_truncated = count_truncated(counts, (size_t)count, R);
    return list_status(w, "contact query", counts, first, count);
}

int rb_query_contacts_dev(rb_world *w, int64_t first, int64_t count, int32_t max_records, int32_t *counts, int32_t *partner,
                          int32_t *kind, void *dist, void *pos, void *frame, int32_t io_dtype) {
    ApiScope api_scope_(w ? w->device : -1);
    WCHK(query_check(w, first, count, max_records, counts, partner, kind, dist, pos, frame));
    if (io_dtype != RB_F64 && io_dtype != RB_F32) return fail(RB_EINVAL, "io_dtype %d is neither RB_F64 nor RB_F32", io_dtype);
    WCHK(query_supported(w));
    if (count == 0) return RB_OK;
    HIPCHK(hipSetDevice(w->device));
    WCHK(dev_ptrs(w->device, "world", {{counts, "counts"}, {partner, "partner"}, {kind, "kind"}, {dist, "dist"}, {pos, "pos"},
                                        {frame, "frame"}}));
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(w->stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(RB_EUNSUPPORTED, "the contact query is not supported under a stream capture");
    if (int rc = finish_pending(w)) return rc;
    WCHK(query_fill(w));
    return query_launch(w, first, count, max_records, counts, partner, kind, dist, pos, frame, io_dtype == RB_F32);
}

int rb_query_impulses(rb_world *w, int64_t first, int64_t count, int32_t max_records, double dt, double restitution,
                      double friction, double contact_threshold, int32_t *counts, int32_t *partner, int32_t *kind, double *dist,
                      double *jn, double *jt, double *vel, double *net, int64_t *n_truncated) {
    ApiScope api_scope_(w ? w->device : -1);
    const int32_t R = max_records;
    WCHK(impulse_check(w, first, count, R, counts, partner, kind, dist, jn, jt, dt, restitution, friction, contact_threshold));
    WCHK(query_supported(w));
    if (n_truncated) *n_truncated = 0;
    if (count == 0) return RB_OK;
    const StageLayout lay = stage_impulses(1, R, vel, net);
    void *const dst[SI_FIELDS] = {dist, jn, jt, vel, net, counts, partner, kind};
    WCHK(staged_ranges(w, lay, "the impulse records", first, count, dst, [&](int64_t at, size_t c, char *d) {
        return impulse_launch(w, at, (int64_t)c, R, dt, restitution, friction, contact_threshold,
                              (int32_t *)lay.at(d, SI_COUNTS, c), (int32_t *)lay.at(d, SI_PARTNER, c),
                              (int32_t *)lay.at(d, SI_KIND, c), lay.at(d, SI_DIST, c), lay.at(d, SI_JN, c), lay.at(d, SI_JT, c),
                              lay.at(d, SI_VEL, c), lay.at(d, SI_NET, c), false);
    }));
    if (n_truncated) *n_truncated = count_truncated(counts, (size_t)count, R);
    return list_status(w, "impulse query", counts, first, count);
}

int rb_query_impulses_dev(rb_world *w, int64_t first, int64_t count, int32_t max_records, double dt, double restitution,
                          double friction, double contact_threshold, int32_t *counts, int32_t *partner, int32_t *kind,
                          void *dist, void *jn, void *jt, void *vel, void *net, int32_t io_dtype) {
    ApiScope api_scope_(w ? w->device : -1);
    WCHK(impulse_check(w, first, count, max_records, counts, partner, kind, dist, jn, jt, dt, restitution, friction,
                       contact_threshold));
    if (io_dtype != RB_F64 && io_dtype != RB_F32) return fail(RB_EINVAL, "io_dtype %d is neither RB_F64 nor RB_F32", io_dtype);
    WCHK(query_supported(w));
    if (count == 0) return RB_OK;
    HIPCHK(hipSetDevice(w->device));
    // (before the pointer attributes are asked for: a capture admits no such call)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(w->stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(RB_EUNSUPPORTED, "the impulse query is not supported under a stream capture");
    WCHK(dev_ptrs(w->device, "world", {{counts, "counts"}, {partner, "partner"}, {kind, "kind"}, {dist, "dist"}, {jn, "jn"},
                                        {jt, "jt"}, {vel, "vel"}, {net, "net"}}));
    if (int rc = finish_pending(w)) return rc;
    WCHK(query_fill(w));
    return impulse_launch(w, first, count, max_records, dt, restitution, friction, contact_threshold, counts, partner, kind,
                          dist, jn, jt, vel, net, io_dtype == RB_F32);
}

}  // extern "C"
