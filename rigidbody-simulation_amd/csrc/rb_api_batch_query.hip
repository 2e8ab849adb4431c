// rb_api_batch_query.hip — the queries of a batch's current state: the contact
// lists (rb_batch_contacts, rb_batch_contacts_dev; kernels in
// rb_batch_contacts.hip, rb_batch_wide.hip, rb_batch_ragged.hip) and the
// impulses of the next step (rb_batch_impulses, rb_batch_impulses_dev; kernels
// in rb_batch_impulses.hip).  They step nothing and write nothing of the batch.
// The device forms enqueue one launch into the caller's arrays.  The host forms
// answer for the listed environments in ranges that fit the batch's staging
// buffer (b->con, laid out by rb_stagelayout.hpp, an environment per unit) and
// download every range straight into the caller's arrays.
#include <cmath>

#include "rb_batch_contacts.hpp"
#include "rb_batch_host.hpp"
#include "rb_batch_impulses.hpp"
#include "rb_stagelayout.hpp"

namespace rb::host {

// ---- the contact query: the arguments both forms share, before any device call ----
static int check_contacts(const rb_batch *b, int32_t R, const void *counts, const void *partner, const void *kind,
                          const void *dist, const void *pos, const void *frame) {
    if (!b) return fail(RB_EINVAL, "null batch");
    if (R < 0) return fail(RB_EINVAL, "max_records < 0");
    if (!counts) return fail(RB_EINVAL, "counts NULL");
    const int given = (partner != nullptr) + (kind != nullptr) + (dist != nullptr);
    if (given != 0 && given != 3) return fail(RB_EINVAL, "partner, kind and dist may be NULL only all together");
    if (R == 0 && (given || pos || frame)) return fail(RB_EINVAL, "max_records 0 with record arrays given");
    if (R > 0 && !given) return fail(RB_EINVAL, "max_records %d with partner, kind and dist NULL (a counts-only query has max_records 0)", R);
    return RB_OK;
}
static int check_contact_law(const rb_batch *b) {
    if (b->law == RB_LAW_BALLS)
        return fail(RB_EUNSUPPORTED, "the two-ball law has no contact list (its hit test carries a tolerance of its own)");
    return RB_OK;
}

// one launch of the query: rows [0, q.n) of q
static int launch_contacts(rb_batch *b, const ContactQuery &q) {
    HIPCHK(by_real(b->dtype, [&](auto t) {
        using T = decltype(t);
        const BatchParams<T> p = batch_params<T>(b, 0, 1.0, 0.0, 0.0, 0.0);
        if (b->pop.set) return launch_ragged_contacts<T>(p, batch_population(b), q, b->pop.boxes, b->stream);
        return b->wide ? launch_batch_wide_contacts<T>(p, q, b->mixed, b->stream)
                       : launch_batch_contacts<T>(p, q, b->mixed, b->stream);
    }));
    return RB_OK;
}

// ---- the impulse query: the arguments both forms share, before any device call:
// the contact query's (jn and jt with the records), rb_batch_step's parameters, finite
static int check_impulses(const rb_batch *b, int32_t R, const void *counts, const void *partner, const void *kind,
                          const void *dist, const void *jn, const void *jt, double dt, double e, double mu, double thr) {
    WCHK(check_contacts(b, R, counts, partner, kind, dist, nullptr, nullptr));
    if ((jn != nullptr) != (partner != nullptr) || (jt != nullptr) != (partner != nullptr))
        return fail(RB_EINVAL, "partner, kind, dist, jn and jt may be NULL only all together (max_records 0)");
    WCHK(batch_check_step(b, 1, dt, e, mu, thr));
    if (!std::isfinite(dt) || !std::isfinite(e) || !std::isfinite(mu) || !std::isfinite(thr))
        return fail(RB_EINVAL, "non-finite step parameters dt=%g e=%g mu=%g thr=%g", dt, e, mu, thr);
    return RB_OK;
}

// one launch of the query: rows [0, q.c.n) of q, by the batch's kind
static int launch_impulses(rb_batch *b, ImpulseQuery q, double dt, double e, double mu, double thr) {
    // (with a population the kinds are the population's: no one-box instance)
    q.c.box = b->box && !b->pop.set;
    HIPCHK(by_real(b->dtype, [&](auto t) {
        using T = decltype(t);
        const BatchParams<T> p = batch_params<T>(b, 1, dt, e, mu, thr);
        if (b->pop.set) return launch_batch_impulses<T>(p, batch_population(b), q, b->pop.boxes, b->stream);
        return launch_batch_impulses<T>(p, Population{}, q, b->mixed, b->stream);
    }));
    return RB_OK;
}

// ---- what the host forms share ----------------------------------------------------
// the listed environments of a host form: n of them, in range, none twice
static int check_query_ids(const rb_batch *b, const int64_t *env_ids, int64_t n) {
    if (n < 0) return fail(RB_EINVAL, "n < 0");
    WCHK(batch_check_ids(b, env_ids, n));
    if (env_ids) {
        std::vector<int64_t> sorted(env_ids, env_ids + n);
        std::sort(sorted.begin(), sorted.end());
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end()) return fail(RB_EINVAL, "env_ids lists environment %lld twice", (long long)*dup);
    }
    return RB_OK;
}

// The host form of a query over n >= 1 listed environments laid out by `lay`
// (`what`: its answers, for the refusal).  One environment must fit the staging
// buffer (refused before any device call); the buffer only grows, to at most
// samp_limit bytes.  The ids go onto the device, then a range of environments
// at a time: launch(first, c) enqueues the query of c environments from `first`
// into the buffer, their arrays that the caller gave (dst, in the layout's order)
// are downloaded, and the stream is waited for: the next range reuses the buffer.
template <typename F>
static int query_ranges(rb_batch *b, const int64_t *env_ids, int64_t n, const StageLayout &lay, const char *what,
                        void *const *dst, F &&launch) {
    const size_t per = lay.per();
    if (per > b->samp_limit)
        return fail(RB_EINVAL, "%s of one environment (%zu bytes) do not fit the staging buffer (%zu bytes: "
                               "RBHIP_BATCH_SAMPLE_BYTES)", what, per, b->samp_limit);
    const int64_t fit = std::min<int64_t>(n, lay.fit(b->samp_limit));
    HIPCHK(hipSetDevice(b->device));
    WCHK(grow((void **)&b->con, &b->con_bytes, per * (size_t)fit));
    if (env_ids) WCHK(batch_put_ids(b, env_ids, n));
    for (int64_t first = 0; first < n; first += fit) {
        const size_t c = (size_t)std::min<int64_t>(fit, n - first);
        WCHK(launch(first, c));
        for (int f = 0; f < lay.n; ++f)
            if (lay.unit[f])
                HIPCHK(hipMemcpyAsync((char *)dst[f] + lay.caller(f, (size_t)first), b->con + lay.offset(f, c), lay.bytes(f, c),
                                      hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
    }
    return RB_OK;
}

// the rows of a range of a host form: listed environments [first, first + c), records of doubles
static void query_rows(const rb_batch *b, const int64_t *env_ids, int64_t first, size_t c, int32_t R, ContactQuery &q) {
    q.ids = env_ids ? b->ids + first : nullptr;
    q.env0 = first;
    q.n = (int64_t)c;
    q.R = R;
}

}  // namespace rb::host

using namespace rb::host;

extern "C" {

int rb_batch_contacts(rb_batch *b, const int64_t *env_ids, int64_t n, int32_t max_records, int32_t *counts,
                      int32_t *partner, int32_t *kind, double *dist, double *pos, double *frame, int64_t *n_truncated) {
    ApiScope api_scope_(b ? b->device : -1);
    const int32_t R = max_records;
    WCHK(check_contacts(b, R, counts, partner, kind, dist, pos, frame));
    WCHK(check_query_ids(b, env_ids, n));
    WCHK(check_contact_law(b));
    if (n_truncated) *n_truncated = 0;
    if (n == 0) return RB_OK;
    const StageLayout lay = stage_contacts((size_t)b->M, R, pos, frame);
    void *const dst[SC_FIELDS] = {dist, pos, frame, counts, partner, kind};
    WCHK(query_ranges(b, env_ids, n, lay, "the contact lists", dst, [&](int64_t first, size_t c) {
        ContactQuery q{};
        char *d = b->con;
        q.counts = (int32_t *)lay.at(d, SC_COUNTS, c); q.partner = (int32_t *)lay.at(d, SC_PARTNER, c);
        q.kind = (int32_t *)lay.at(d, SC_KIND, c);
        q.dist = lay.at(d, SC_DIST, c); q.pos = lay.at(d, SC_POS, c); q.frame = lay.at(d, SC_FRAME, c);
        query_rows(b, env_ids, first, c, R, q);
        q.box = b->box;
        return launch_contacts(b, q);
    }));
    if (n_truncated) *n_truncated = count_truncated(counts, (size_t)n * (size_t)b->M, R);
    return RB_OK;
}

int rb_batch_contacts_dev(rb_batch *b, int32_t max_records, int32_t *counts, int32_t *partner, int32_t *kind,
                          void *dist, void *pos, void *frame, int32_t io_dtype) {
    ApiScope api_scope_(b ? b->device : -1);
    WCHK(check_contacts(b, max_records, counts, partner, kind, dist, pos, frame));
    WCHK(batch_check_io(io_dtype));
    WCHK(check_contact_law(b));
    HIPCHK(hipSetDevice(b->device));
    WCHK(dev_ptrs(b->device, "batch", {{counts, "counts"}, {partner, "partner"}, {kind, "kind"}, {dist, "dist"}, {pos, "pos"},
                                       {frame, "frame"}}));
    ContactQuery q{};
    q.counts = counts; q.partner = partner; q.kind = kind;
    q.dist = dist; q.pos = pos; q.frame = frame;
    q.n = b->E; q.R = max_records;
    q.io32 = io_dtype == RB_F32;
    q.box = b->box;
    return launch_contacts(b, q);
}

int rb_batch_impulses(rb_batch *b, const int64_t *env_ids, int64_t n, int32_t max_records, double dt, double restitution,
                      double friction, double contact_threshold, int32_t *counts, int32_t *partner, int32_t *kind,
                      double *dist, double *jn, double *jt, double *vel, double *net, int64_t *n_truncated) {
    ApiScope api_scope_(b ? b->device : -1);
    const int32_t R = max_records;
    WCHK(check_impulses(b, R, counts, partner, kind, dist, jn, jt, dt, restitution, friction, contact_threshold));
    WCHK(check_query_ids(b, env_ids, n));
    WCHK(check_contact_law(b));
    if (n_truncated) *n_truncated = 0;
    if (n == 0) return RB_OK;
    const StageLayout lay = stage_impulses((size_t)b->M, R, vel, net);
    void *const dst[SI_FIELDS] = {dist, jn, jt, vel, net, counts, partner, kind};
    WCHK(query_ranges(b, env_ids, n, lay, "the impulse records", dst, [&](int64_t first, size_t c) {
        ImpulseQuery q{};
        char *d = b->con;
        q.c.counts = (int32_t *)lay.at(d, SI_COUNTS, c); q.c.partner = (int32_t *)lay.at(d, SI_PARTNER, c);
        q.c.kind = (int32_t *)lay.at(d, SI_KIND, c);
        q.c.dist = lay.at(d, SI_DIST, c); q.jn = lay.at(d, SI_JN, c); q.jt = lay.at(d, SI_JT, c);
        q.vel = lay.at(d, SI_VEL, c); q.net = lay.at(d, SI_NET, c);
        query_rows(b, env_ids, first, c, R, q.c);
        return launch_impulses(b, q, dt, restitution, friction, contact_threshold);
    }));
    if (n_truncated) *n_truncated = count_truncated(counts, (size_t)n * (size_t)b->M, R);
    return RB_OK;
}

int rb_batch_impulses_dev(rb_batch *b, int32_t max_records, double dt, double restitution, double friction,
                          double contact_threshold, int32_t *counts, int32_t *partner, int32_t *kind, void *dist, void *jn,
                          void *jt, void *vel, void *net, int32_t io_dtype) {
    ApiScope api_scope_(b ? b->device : -1);
    WCHK(check_impulses(b, max_records, counts, partner, kind, dist, jn, jt, dt, restitution, friction, contact_threshold));
    WCHK(batch_check_io(io_dtype));
    WCHK(check_contact_law(b));
    HIPCHK(hipSetDevice(b->device));
    WCHK(dev_ptrs(b->device, "batch", {{counts, "counts"}, {partner, "partner"}, {kind, "kind"}, {dist, "dist"}, {jn, "jn"}, {jt, "jt"},
                            {vel, "vel"}, {net, "net"}}));
    ImpulseQuery q{};
    q.c.counts = counts; q.c.partner = partner; q.c.kind = kind;
    q.c.dist = dist; q.jn = jn; q.jt = jt; q.vel = vel; q.net = net;
    q.c.n = b->E; q.c.R = max_records;
    q.c.io32 = io_dtype == RB_F32;
    return launch_impulses(b, q, dt, restitution, friction, contact_threshold);
}

}  // extern "C"
