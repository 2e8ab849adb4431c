// rb_api_batch.hip — batched worlds: lifetime (rb_batch_create*,
// rb_batch_destroy), the setters (rb_batch_set_params / _bodies / _population /
// _contact_law / _planes / _gravity / _xfrc), rb_batch_set_state and
// rb_batch_get_state, rb_batch_step, rb_batch_run_sampled,
// rb_batch_run_sampled_impulses and rb_batch_status.
// Kernels: rb_batch.hip, rb_batch_boxes.hip and, for an environment of more
// than 64 bodies, rb_batch_wide.hip; with a population set, rb_batch_ragged.hip;
// a sampled run that records impulse curves, rb_batch_sensed.hip.
// E replicas of a template environment of M <= 256 bodies, body b of
// environment e at slot e * M + b of every device row.  All work is enqueued
// on the batch's stream (its own, or the caller's: rb_batch_set_stream); the
// entries here take host arrays and return after it finished.  The
// device-resident boundary is rb_api_batch_dev.hip, the queries of the state
// rb_api_batch_query.hip; rb_batch_host.hpp holds what the three share.
#include <cmath>

#include "rb_batch_host.hpp"
#include "rb_laneplan.hpp"

using namespace rb::host;

static_assert(BATCH_EDOM == RB_EDOM && BATCH_CHUNK == RB_BATCH_CHUNK && BATCH_WIDE_MAX == RB_BATCH_MAX_BODIES, "batch constants");

namespace {

void free_batch(rb_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->own_stream) (void)hipStreamSynchronize(b->stream);
    void *bufs[] = {b->snap, b->state, b->consts, b->env_e, b->env_mu, b->code, b->count, b->steps_done,
                    b->io_q, b->io_v, b->ids, b->samp, b->env_planes, b->env_g, b->env_xfrc, b->d_kind, b->refused, b->con, b->sense, b->pop.tables};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    if (b->own_stream) (void)hipStreamDestroy(b->own_stream);   // (never the caller's)
    delete b;
}

int bput(rb_batch *b, void *dst, const void *src, size_t bytes) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return RB_OK;
}

double batch_bound_of(int32_t kind, const double *s) {
    return kind == RB_BODY_SPHERE ? s[0] : sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
}

// the kind of body slot g: the population's, else the template's
int32_t batch_kind_of(const rb_batch *b, int64_t g) {
    return b->pop.set ? b->pop.kind[(size_t)g] : b->kind[(size_t)(g % b->M)];
}
// is body slot g stepped (a present body)?
bool batch_present(const rb_batch *b, int64_t g) { return !b->pop.set || g % b->M < b->pop.n[(size_t)(g / b->M)]; }

// the cell size of a world of these bodies (upload_consts; under the two-ball
// law rb_set_contact_law's, from the reach 2 rmax + tol): the position check
// of a step uses the same predicate
void batch_set_cell(rb_batch *b) {
    if (b->law == RB_LAW_BALLS) {
        const double reach = 2.0 * b->rmax + b->tol;
        b->inv_cs = 1.0 / (reach > 0 ? 2.0 * reach * 1.001 : 1.0);
    } else {
        b->inv_cs = 1.0 / (b->rmax > 0 ? 4.0 * b->rmax * 1.001 : 1.0);
    }
}

// row r (of the 8 constant rows) <- src[slot * stride + off], as the batch's real type
int batch_put_row(rb_batch *b, int row, const double *src, int stride, int off) {
    return by_real(b->dtype, [&](auto t) {
        using T = decltype(t);
        std::vector<T> h((size_t)b->N);
        for (int64_t g = 0; g < b->N; ++g) h[(size_t)g] = (T)src[(size_t)g * stride + off];
        return bput(b, dp<T>(b->consts, row * b->N), h.data(), sizeof(T) * h.size());
    });
}

// A per-environment array into its device rows (rb_batch_set_planes / _gravity
// / _xfrc): src is [units][width] doubles, the device copy `width` rows of
// `units` reals (struct-of-arrays, as the batch's real type), allocated on
// first use.  Nothing of the batch changes unless every step succeeds.
int batch_put_env(rb_batch *b, void **buf, bool *have, const double *src, int64_t units, int width) {
    HIPCHK(hipSetDevice(b->device));
    if (!src) {
        *have = false;
        return RB_OK;
    }
    const size_t n = (size_t)units * (size_t)width;
    void *dst = *buf;
    if (!dst) HIPCHK(hipMalloc(&dst, n * (size_t)b->esz));
    const int rc = by_real(b->dtype, [&](auto t) {
        using T = decltype(t);
        std::vector<T> h(n);
        for (int64_t u = 0; u < units; ++u)
            for (int d = 0; d < width; ++d) h[(size_t)d * (size_t)units + (size_t)u] = (T)src[(size_t)u * width + d];
        return bput(b, dst, h.data(), sizeof(T) * n);
    });
    if (rc != RB_OK) {
        if (!*buf) (void)hipFree(dst);
        return rc;
    }
    *buf = dst;
    *have = true;
    return RB_OK;
}

// The bounding radius of every body slot from the sizes last given and the
// slot's kind, and the batch's largest radius over the bodies that are
// stepped (an absent slot keeps a radius, which nothing reads).
int batch_put_bounds(rb_batch *b) {
    std::vector<double> bound((size_t)b->N);
    double rmax = 0;
    for (int64_t g = 0; g < b->N; ++g) {
        bound[(size_t)g] = batch_bound_of(batch_kind_of(b, g), b->size.data() + 3 * g);
        if (batch_present(b, g) && bound[(size_t)g] > rmax) rmax = bound[(size_t)g];
    }
    WCHK(batch_put_row(b, 7, bound.data(), 1, 0));
    b->rmax = rmax;
    batch_set_cell(b);
    // the snapshots carry the bounding radius
    HIPCHK(by_real(b->dtype, [&](auto t) {
        using T = decltype(t);
        return launch_batch_bound<T>(dp<Snap<T>>(b->snap, 0), dp<T>(b->consts, 7 * b->N), b->N, b->stream);
    }));
    HIPCHK(hipStreamSynchronize(b->stream));
    return RB_OK;
}

template <typename T> StateIO<T> batch_io(rb_batch *b) {
    StateIO<T> p{};
    p.qpos = b->io_q;
    p.qvel = b->io_v;
    p.snap = dp<Snap<T>>(b->snap, 0);
    p.quat = nullptr;
    p.st = BodyState<T>{dp<T>(b->state, 0), b->N};
    p.bound = dp<T>(b->consts, 7 * b->N);
    p.N = b->N;
    p.lo = 0;
    p.n_local = (int32_t)b->N;
    p.balls = 0;
    return p;
}

// bytes one sample of the batch takes in the sample buffer: its slot (rounded
// up to whole doubles, so that the boundary rows behind the slots are aligned)
// and its boundary rows
size_t align8(size_t n) { return (n + 7) & ~(size_t)7; }
size_t sample_bytes(const rb_batch *b, int rows) {
    const size_t vals = (size_t)b->N * (size_t)rows;
    return align8(vals * (size_t)b->esz) + vals * sizeof(double);
}

// the listed environments' rows: staging of n * M rows and the ids on the device
int batch_stage(rb_batch *b, const int64_t *env_ids, int64_t n) {
    const size_t rows = (size_t)(n * b->M);
    WCHK(grow((void **)&b->io_q, &b->io_q_bytes, sizeof(double) * 7 * rows));
    WCHK(grow((void **)&b->io_v, &b->io_v_bytes, sizeof(double) * 6 * rows));
    if (env_ids) WCHK(batch_put_ids(b, env_ids, n));
    return RB_OK;
}

// rb_batch_create / rb_batch_create_mixed / rb_batch_create_wide (mixed: a box
// among several bodies is accepted; max_bodies: the entry's bound on n_bodies)
int batch_create(rb_batch **out, const rb_scene_desc *d, int64_t n_envs, bool mixed, int max_bodies = BATCH_BLOCK) {
    if (!out || !d) return fail(RB_EINVAL, "null argument");
    *out = nullptr;
    if (n_envs < 1) return fail(RB_EINVAL, "n_envs must be >= 1");
    if (d->n_bodies < 1 || d->n_bodies > max_bodies)
        return fail(RB_EINVAL, "n_bodies (bodies per environment) must be in [1, %d]", max_bodies);
    if (d->world_size != 1 || d->rank != 0) return fail(RB_EINVAL, "a batch is not sharded: world_size must be 1, rank 0");
    if (n_envs > ((int64_t)INT32_MAX / 2) / d->n_bodies) return fail(RB_EINVAL, "n_envs * n_bodies out of range");
    if (d->n_planes < 0 || d->n_planes > RB_MAX_PLANES) return fail(RB_EINVAL, "n_planes must be in [0, %d]", RB_MAX_PLANES);
    if (d->dtype != RB_F64 && d->dtype != RB_F32) return fail(RB_EINVAL, "dtype must be RB_F64 or RB_F32");
    if (!d->kind || !d->mass || !d->inertia || !d->size || (d->n_planes && !d->planes))
        return fail(RB_EINVAL, "null scene array");
    if (d->normal_convention != RB_NORMAL_ORIENTED && d->normal_convention != RB_NORMAL_RAW)
        return fail(RB_EINVAL, "bad normal_convention");
    bool any_box = false;
    for (int64_t k = 0; k < d->n_bodies; ++k) {
        if (d->kind[k] != RB_BODY_SPHERE && d->kind[k] != RB_BODY_BOX) return fail(RB_EINVAL, "body %lld: bad kind", (long long)k);
        if (!(d->mass[k] > 0)) return fail(RB_EINVAL, "body %lld: mass must be > 0", (long long)k);
        any_box = any_box || d->kind[k] == RB_BODY_BOX;
    }
    if (any_box && d->n_bodies > 1 && !mixed)
        return fail(RB_EUNSUPPORTED, "rb_batch: unsupported template: a box body in an environment of more than one body "
                                     "(box-involved pairs are stepped by rb_batch_create_mixed, or by rb_world)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(RB_ENODEV, "no HIP device available");
    if (d->device < 0 || d->device >= ndev) return fail(RB_ENODEV, "device %d out of range (have %d)", d->device, ndev);

    rb_batch *b = new rb_batch();
    b->dtype = d->dtype;
    b->esz = d->dtype == RB_F64 ? 8 : 4;
    b->device = d->device;
    b->E = n_envs;
    b->M = (int32_t)d->n_bodies;
    b->N = b->E * b->M;
    b->mixed = any_box && d->n_bodies > 1;
    b->box = any_box && !b->mixed;
    b->wide = d->n_bodies > BATCH_BLOCK;
    b->kind.assign(d->kind, d->kind + d->n_bodies);
    b->n_planes = d->n_planes;
    for (int k = 0; k < d->n_planes; ++k)
        for (int j = 0; j < 6; ++j) b->planes[k][j] = d->planes[6 * k + j];
    for (int j = 0; j < 3; ++j) b->g[j] = d->gravity[j];
    b->oriented = d->normal_convention == RB_NORMAL_ORIENTED;
    if (const char *ev = getenv("RBHIP_BATCH_SAMPLE_BYTES"))
        if (atoll(ev) > 0) b->samp_limit = (size_t)atoll(ev);
    auto bail = [&](int rc) { free_batch(b); return rc; };
    if (hipSetDevice(b->device) != hipSuccess) return bail(fail(RB_ENODEV, "hipSetDevice(%d) failed", b->device));
    if (hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(RB_ENODEV, "hipStreamCreate failed"));
    b->stream = b->own_stream;
    const size_t esz = (size_t)b->esz, N = (size_t)b->N, E = (size_t)b->E;
    const std::pair<void **, size_t> allocs[] = {
        {&b->snap, esz * 4 * N}, {&b->state, esz * 13 * N}, {&b->consts, esz * 8 * N},
        {&b->env_e, esz * E}, {&b->env_mu, esz * E}, {(void **)&b->code, sizeof(int32_t) * E},
        {(void **)&b->count, sizeof(int32_t)}, {(void **)&b->steps_done, sizeof(int64_t) * E}};
    for (const auto &a : allocs) {
        if (hipMalloc(a.first, a.second) != hipSuccess) return bail(fail(RB_ENOMEM, "hipMalloc(%zu) failed", a.second));
        if (hipMemsetAsync(*a.first, 0, a.second, b->stream) != hipSuccess) return bail(fail(RB_ENODEV, "hipMemsetAsync failed"));
    }
    if (hipMalloc((void **)&b->refused, sizeof(uint32_t)) != hipSuccess) return bail(fail(RB_ENOMEM, "hipMalloc(4) failed"));
    if (hipMemsetAsync(b->refused, 0xff, sizeof(uint32_t), b->stream) != hipSuccess)
        return bail(fail(RB_ENODEV, "hipMemsetAsync failed"));
    if (b->mixed) {
        const size_t kb = sizeof(int32_t) * (size_t)b->M;
        if (hipMalloc((void **)&b->d_kind, kb) != hipSuccess) return bail(fail(RB_ENOMEM, "hipMalloc(%zu) failed", kb));
        if (int rc = bput(b, b->d_kind, b->kind.data(), kb)) return bail(rc);
    }
    // the template's constants, replicated per environment
    std::vector<double> mass(N), inertia(3 * N), size(3 * N);
    for (size_t g = 0; g < N; ++g) {
        const size_t k = g % (size_t)b->M;
        mass[g] = d->mass[k];
        for (int j = 0; j < 3; ++j) { inertia[3 * g + j] = d->inertia[3 * k + j]; size[3 * g + j] = d->size[3 * k + j]; }
    }
    if (int rc = rb_batch_set_bodies(b, mass.data(), inertia.data(), size.data())) return bail(rc);
    *out = b;
    return RB_OK;
}

}  // namespace

namespace rb::host {

int batch_check_step(const rb_batch *b, int64_t nsteps, double dt, double e, double mu, double thr) {
    if (!b) return fail(RB_EINVAL, "null batch");
    if (nsteps < 0) return fail(RB_EINVAL, "nsteps < 0");
    if (!(dt > 0) || !(e >= 0) || !(mu >= 0) || !(thr >= 0))
        return fail(RB_EINVAL, "invalid step parameters dt=%g e=%g mu=%g thr=%g", dt, e, mu, thr);
    return RB_OK;
}

// the environments failed so far, as rb_batch_step reports them
int batch_report(rb_batch *b, int64_t *n_failed) {
    int32_t cnt = 0;
    HIPCHK(hipMemsetAsync(b->count, 0, sizeof(int32_t), b->stream));
    HIPCHK(launch_batch_count(b->code, b->E, b->count, b->stream));
    HIPCHK(hipMemcpyAsync(&cnt, b->count, sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (n_failed) {
        *n_failed = cnt;
        return RB_OK;
    }
    if (cnt > 0)
        return fail(RB_EDOM, "device: non-finite or out-of-range body position in %d environment(s) (rb_batch_status)", cnt);
    return RB_OK;
}

// an env_ids list onto the device (b->ids)
int batch_put_ids(rb_batch *b, const int64_t *env_ids, int64_t n) {
    WCHK(grow((void **)&b->ids, &b->ids_bytes, sizeof(int64_t) * (size_t)n));
    HIPCHK(hipMemcpyAsync(b->ids, env_ids, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, b->stream));
    return RB_OK;
}

// env_ids == NULL: all environments (n must be n_envs); else n distinct ids in range
int batch_check_ids(const rb_batch *b, const int64_t *env_ids, int64_t n) {
    if (!env_ids) return n == b->E ? RB_OK : fail(RB_EINVAL, "env_ids NULL: n must be n_envs (%lld)", (long long)b->E);
    if (n < 0) return fail(RB_EINVAL, "n < 0");
    for (int64_t k = 0; k < n; ++k)
        if (env_ids[k] < 0 || env_ids[k] >= b->E)
            return fail(RB_EINVAL, "env_ids[%lld] = %lld outside [0, %lld)", (long long)k, (long long)env_ids[k], (long long)b->E);
    return RB_OK;
}

}  // namespace rb::host

extern "C" {

int rb_batch_create(rb_batch **out, const rb_scene_desc *d, int64_t n_envs) {
    ApiScope api_scope_(d ? d->device : -1);
    return batch_create(out, d, n_envs, false);
}

int rb_batch_create_mixed(rb_batch **out, const rb_scene_desc *d, int64_t n_envs) {
    ApiScope api_scope_(d ? d->device : -1);
    return batch_create(out, d, n_envs, true);
}

int rb_batch_create_wide(rb_batch **out, const rb_scene_desc *d, int64_t n_envs) {
    ApiScope api_scope_(d ? d->device : -1);
    return batch_create(out, d, n_envs, true, BATCH_WIDE_MAX);
}

void rb_batch_destroy(rb_batch *b) {
    ApiScope api_scope_(b ? b->device : -1);
    free_batch(b);
}

int rb_batch_set_params(rb_batch *b, const double *restitution, const double *friction) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    for (int64_t e = 0; e < b->E; ++e)
        if ((restitution && !(restitution[e] >= 0)) || (friction && !(friction[e] >= 0)))
            return fail(RB_EINVAL, "environment %lld: restitution and friction must be >= 0", (long long)e);
    HIPCHK(hipSetDevice(b->device));
    const double *src[2] = {restitution, friction};
    void *dst[2] = {b->env_e, b->env_mu};
    for (int k = 0; k < 2; ++k) {
        if (!src[k]) continue;
        WCHK(by_real(b->dtype, [&](auto t) {
            const std::vector<decltype(t)> f(src[k], src[k] + b->E);
            return bput(b, dst[k], f.data(), sizeof(f[0]) * f.size());
        }));
    }
    b->have_e = restitution != nullptr;
    b->have_mu = friction != nullptr;
    return RB_OK;
}

int rb_batch_set_bodies(rb_batch *b, const double *mass, const double *inertia, const double *size) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    if (mass)
        for (int64_t g = 0; g < b->N; ++g)
            if (!(mass[g] > 0)) return fail(RB_EINVAL, "body slot %lld: mass must be > 0", (long long)g);
    HIPCHK(hipSetDevice(b->device));
    if (mass) WCHK(batch_put_row(b, 0, mass, 1, 0));
    if (inertia)
        for (int j = 0; j < 3; ++j) WCHK(batch_put_row(b, 1 + j, inertia, 3, j));
    if (size) {
        for (int j = 0; j < 3; ++j) WCHK(batch_put_row(b, 4 + j, size, 3, j));
        b->size.assign(size, size + 3 * (size_t)b->N);
        WCHK(batch_put_bounds(b));
    }
    return RB_OK;
}

int rb_batch_set_population(rb_batch *b, const int32_t *n_bodies, const int32_t *kind) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    const bool set = n_bodies || kind;
    if (n_bodies)
        for (int64_t e = 0; e < b->E; ++e)
            if (n_bodies[e] < 1 || n_bodies[e] > b->M)
                return fail(RB_EINVAL, "environment %lld: a body count of %d is outside [1, %d]", (long long)e, n_bodies[e], b->M);
    if (kind)
        for (int64_t g = 0; g < b->N; ++g)
            if (kind[g] != RB_BODY_SPHERE && kind[g] != RB_BODY_BOX)
                return fail(RB_EINVAL, "environment %lld, body %lld: bad kind %d", (long long)(g / b->M),
                            (long long)(g % b->M), kind[g]);
    if (set && b->law == RB_LAW_BALLS)
        return fail(RB_EUNSUPPORTED, "the two-ball law takes no population: its batches are uniform");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));         // pending work finishes under the population it was enqueued with
    // the new population, complete before the batch changes
    rb_batch::Pop next;
    next.set = set;
    if (set) {
        if (n_bodies) next.n.assign(n_bodies, n_bodies + b->E);
        else next.n.assign((size_t)b->E, b->M);
        if (kind) next.kind.assign(kind, kind + b->N);
        else
            for (int64_t g = 0; g < b->N; ++g) next.kind.push_back(b->kind[(size_t)(g % b->M)]);
        for (int64_t g = 0; g < b->N; ++g) {
            const bool present = g % b->M < next.n[(size_t)(g / b->M)];
            next.boxes = next.boxes || (present && next.kind[(size_t)g] == RB_BODY_BOX);
            next.absent = next.absent || !present;
        }
        std::vector<int32_t> h(next.n);
        h.insert(h.end(), next.kind.begin(), next.kind.end());
        if (!b->wide) {
            LanePlan plan;
            if (!lane_plan(next.n.data(), b->E, b->M, plan)) return fail(RB_EINVAL, "no lane plan for this population");
            h.insert(h.end(), plan.wave_env0.begin(), plan.wave_env0.end());
            h.insert(h.end(), plan.lane_row.begin(), plan.lane_row.end());
            next.waves = plan.waves;
            next.epw = plan.epw_max;
        }
        HIPCHK(hipMalloc((void **)&next.tables, sizeof(int32_t) * h.size()));
        if (int rc = bput(b, next.tables, h.data(), sizeof(int32_t) * h.size())) {
            (void)hipFree(next.tables);
            return rc;
        }
    }
    // commit by swap (`next` then holds the old population); the bounding radii follow the kinds
    const double was_rmax = b->rmax;
    std::swap(b->pop, next);
    const int rc = batch_put_bounds(b);
    if (rc != RB_OK) {
        // (a device error; the host side is put back, and so are the radii, where the device still answers)
        std::swap(b->pop, next);
        b->rmax = was_rmax;
        (void)batch_put_bounds(b);
    }
    if (next.tables) (void)hipFree(next.tables);   // the tables of the population that lost
    return rc;
}

int rb_batch_set_state(rb_batch *b, const int64_t *env_ids, int64_t n, const double *qpos, const double *qvel) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b || !qpos || !qvel) return fail(RB_EINVAL, "null argument");
    WCHK(batch_check_ids(b, env_ids, n));
    if (n == 0) return RB_OK;
    HIPCHK(hipSetDevice(b->device));
    WCHK(batch_stage(b, env_ids, n));
    const size_t rows = (size_t)(n * b->M);
    HIPCHK(hipMemcpyAsync(b->io_q, qpos, sizeof(double) * 7 * rows, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->io_v, qvel, sizeof(double) * 6 * rows, hipMemcpyHostToDevice, b->stream));
    HIPCHK(by_real(b->dtype, [&](auto t) {
        using T = decltype(t);
        return env_ids ? launch_batch_state_in<T>(batch_io<T>(b), b->ids, n, b->M, b->stream)
                       : launch_state_in<T>(batch_io<T>(b), b->stream);
    }));
    HIPCHK(launch_batch_reset(b->code, b->steps_done, env_ids ? b->ids : nullptr, n, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return RB_OK;
}

int rb_batch_get_state(rb_batch *b, const int64_t *env_ids, int64_t n, double *qpos, double *qvel) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b || (!qpos && !qvel)) return fail(RB_EINVAL, "null argument");
    WCHK(batch_check_ids(b, env_ids, n));
    if (n == 0) return RB_OK;
    HIPCHK(hipSetDevice(b->device));
    WCHK(batch_stage(b, env_ids, n));
    HIPCHK(by_real(b->dtype, [&](auto t) {
        using T = decltype(t);
        return env_ids ? launch_batch_state_out<T>(batch_io<T>(b), b->ids, n, b->M, b->stream)
                       : launch_state_out<T>(batch_io<T>(b), true, true, b->stream);
    }));
    const size_t rows = (size_t)(n * b->M);
    if (qpos) HIPCHK(hipMemcpyAsync(qpos, b->io_q, sizeof(double) * 7 * rows, hipMemcpyDeviceToHost, b->stream));
    if (qvel) HIPCHK(hipMemcpyAsync(qvel, b->io_v, sizeof(double) * 6 * rows, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return RB_OK;
}

int rb_batch_set_contact_law(rb_batch *b, int32_t law, double tol) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    if (law != RB_LAW_MUJOCO && law != RB_LAW_BALLS) return fail(RB_EINVAL, "unknown contact law %d", law);
    if (!(tol >= 0) || !(tol < 1e6)) return fail(RB_EINVAL, "tol must be finite and >= 0");
    if (law == RB_LAW_BALLS) {
        if (b->pop.set)
            return fail(RB_EUNSUPPORTED, "the two-ball law takes no population (clear it first: rb_batch_set_population "
                                         "with NULL, NULL)");
        if (b->box || b->mixed) return fail(RB_EUNSUPPORTED, "the two-ball law takes spheres only");
        if (b->wide)
            return fail(RB_EUNSUPPORTED, "the two-ball law takes environments of at most %d bodies (this one has %d)",
                        BATCH_BLOCK, b->M);
        const double ground[6] = {0, 0, 1, 0, 0, 0};
        if (b->n_planes > 1 || (b->n_planes == 1 && memcmp(b->planes[0], ground, sizeof(ground)) != 0))
            return fail(RB_EUNSUPPORTED, "the two-ball law's only plane is the z = 0 ground (ball_collision.py:88-90)");
        if (b->have_planes || b->have_xfrc)
            return fail(RB_EUNSUPPORTED, "the two-ball law takes no per-environment planes or applied forces "
                                         "(clear them first: rb_batch_set_planes / rb_batch_set_xfrc with NULL)");
    }
    // both laws keep a ball's true position in the snapshots and neither
    // caches anything between launches: a switch converts nothing
    b->law = law;
    b->tol = tol;
    batch_set_cell(b);
    return RB_OK;
}

int rb_batch_set_planes(rb_batch *b, const double *planes) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    if (planes) {
        if (b->n_planes == 0) return fail(RB_EINVAL, "the template has no plane: the plane count is the template's");
        for (int64_t e = 0; e < b->E; ++e)
            for (int k = 0; k < b->n_planes; ++k)
                for (int j = 0; j < 6; ++j)
                    if (!std::isfinite(planes[((size_t)e * b->n_planes + k) * 6 + j]))
                        return fail(RB_EINVAL, "environment %lld, plane %d: non-finite value", (long long)e, k);
        if (b->law == RB_LAW_BALLS)
            return fail(RB_EUNSUPPORTED, "the two-ball law's only plane is the z = 0 ground: no per-environment planes");
    }
    // [E][n_planes * 6] -> n_planes * 6 rows of E
    return batch_put_env(b, &b->env_planes, &b->have_planes, planes, b->E, b->n_planes * 6);
}

int rb_batch_set_gravity(rb_batch *b, const double *gravity) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    if (gravity)
        for (int64_t e = 0; e < b->E; ++e)
            for (int j = 0; j < 3; ++j)
                if (!std::isfinite(gravity[3 * e + j]))
                    return fail(RB_EINVAL, "environment %lld: non-finite gravity", (long long)e);
    return batch_put_env(b, &b->env_g, &b->have_g, gravity, b->E, 3);
}

int rb_batch_set_xfrc(rb_batch *b, const double *xfrc) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    if (xfrc) {
        for (int64_t g = 0; g < b->N; ++g)
            for (int j = 0; j < 6; ++j)
                if (!std::isfinite(xfrc[6 * g + j]))
                    return fail(RB_EINVAL, "environment %lld, body %lld: non-finite applied force or torque",
                                (long long)(g / b->M), (long long)(g % b->M));
        if (b->law == RB_LAW_BALLS)
            return fail(RB_EUNSUPPORTED, "the two-ball law takes no applied forces (ball_collision.py:73-125)");
    }
    return batch_put_env(b, &b->env_xfrc, &b->have_xfrc, xfrc, b->N, 6);
}

int rb_batch_step(rb_batch *b, int64_t nsteps, double dt, double e, double mu, double thr, int64_t *n_failed) {
    ApiScope api_scope_(b ? b->device : -1);
    WCHK(batch_check_step(b, nsteps, dt, e, mu, thr));
    HIPCHK(hipSetDevice(b->device));
    WCHK(batch_enqueue_steps(b, nsteps, dt, e, mu, thr));
    return batch_report(b, n_failed);
}

int rb_batch_run_sampled(rb_batch *b, int64_t nsteps, int64_t every, double dt, double e, double mu, double thr,
                         double *qpos, double *qvel, int64_t *n_failed) {
    ApiScope api_scope_(b ? b->device : -1);
    SampledRun r;
    WCHK(batch_sampled_prelude(b, nsteps, every, dt, e, mu, thr, qpos, qvel, nullptr, sample_bytes, r));
    // the slots first, the boundary rows of `fit` samples behind them
    const size_t N = (size_t)b->N, fit = (size_t)r.fit;
    const int rows = r.rows;
    char *slots = b->samp;
    double *out_q = reinterpret_cast<double *>(b->samp + align8(fit * N * rows * b->esz));
    double *out_v = out_q + fit * N * 7;

    SamplePlan plan(nsteps, every, BATCH_CHUNK, r.fit);
    SampleLaunch l;
    while (plan.next(l)) {
        WCHK(batch_enqueue_sampled(b, l, slots, r, every, dt, e, mu, thr));
        if (l.drain == 0) continue;
        // a plain synchronous drain: transpose, download, wait
        HIPCHK(by_real(b->dtype, [&](auto t) {
            using T = decltype(t);
            return launch_batch_samples_out<T>(reinterpret_cast<const T *>(slots), 0, (int32_t)l.drain, rows, b->N, out_q,
                                               out_v, b->stream);
        }));
        const size_t n = (size_t)l.drain * N, at = (size_t)l.drain_at * N;
        HIPCHK(hipMemcpyAsync(qpos + 7 * at, out_q, sizeof(double) * 7 * n, hipMemcpyDeviceToHost, b->stream));
        if (qvel) HIPCHK(hipMemcpyAsync(qvel + 6 * at, out_v, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
    }
    return batch_report(b, n_failed);
}

int rb_batch_run_sampled_impulses(rb_batch *b, int64_t nsteps, int64_t every, double dt, double e, double mu, double thr,
                                  double *qpos, double *qvel, double *net, int64_t *n_failed) {
    ApiScope api_scope_(b ? b->device : -1);
    SampledRun r;
    WCHK(batch_sensed_prelude(b, nsteps, every, dt, e, mu, thr, qpos, qvel, net, nullptr, sample_bytes, r));
    if (nsteps / every == 0) {         // no window: nothing to sense
        WCHK(batch_enqueue_steps(b, nsteps, dt, e, mu, thr));
        return batch_report(b, n_failed);
    }
    // the slots first, the boundary rows of `fit` samples behind them: qpos, qvel (those asked for), net
    const size_t N = (size_t)b->N, fit = (size_t)r.fit;
    const int rows = r.rows;
    char *slots = b->samp;
    double *out = reinterpret_cast<double *>(b->samp + align8(fit * N * rows * b->esz));
    double *out_q = qpos ? out : nullptr;
    double *out_v = qvel ? out + fit * N * (qpos ? 7 : 0) : nullptr;
    double *out_n = out + fit * N * (size_t)(rows - 6);
    const SensedRun sr = batch_sensed_run(b, qpos != nullptr, qvel != nullptr);
    HIPCHK(hipMemsetAsync(b->sense, 0, N * 6 * (size_t)b->esz, b->stream));   // the first window starts from +0

    SamplePlan plan(nsteps, every, BATCH_CHUNK, r.fit);
    SampleLaunch l;
    while (plan.next(l)) {
        WCHK(batch_enqueue_sensed(b, l, slots, r, sr, every, dt, e, mu, thr));
        if (l.drain == 0) continue;
        // a plain synchronous drain: transpose, download, wait
        HIPCHK(by_real(b->dtype, [&](auto t) {
            using T = decltype(t);
            return launch_sensed_out<T, double>(reinterpret_cast<const T *>(slots), (int32_t)l.drain, rows, sr, b->N, out_q,
                                                out_v, out_n, b->stream);
        }));
        const size_t n = (size_t)l.drain * N, at = (size_t)l.drain_at * N;
        if (qpos) HIPCHK(hipMemcpyAsync(qpos + 7 * at, out_q, sizeof(double) * 7 * n, hipMemcpyDeviceToHost, b->stream));
        if (qvel) HIPCHK(hipMemcpyAsync(qvel + 6 * at, out_v, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipMemcpyAsync(net + 6 * at, out_n, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
    }
    return batch_report(b, n_failed);
}

int rb_batch_status(rb_batch *b, int32_t *code, int64_t *steps_done) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b || (!code && !steps_done)) return fail(RB_EINVAL, "null argument");
    HIPCHK(hipSetDevice(b->device));
    if (code) HIPCHK(hipMemcpyAsync(code, b->code, sizeof(int32_t) * (size_t)b->E, hipMemcpyDeviceToHost, b->stream));
    if (steps_done)
        HIPCHK(hipMemcpyAsync(steps_done, b->steps_done, sizeof(int64_t) * (size_t)b->E, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return RB_OK;
}

}  // extern "C"
