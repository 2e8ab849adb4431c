// rb_api_batch.hip — batched worlds (rb_batch_*; kernels in rb_batch.hip,
// rb_batch_boxes.hip and, for an environment of more than 64 bodies,
// rb_batch_wide.hip; with a population set, rb_batch_ragged.hip).
// E replicas of a template environment of M <= 256 bodies, body b of
// environment e at slot e * M + b of every device row.  All work is enqueued
// on the batch's stream (its own, or the caller's: rb_batch_set_stream); the
// entries that take host arrays return after it finished, the device-resident
// boundary (rb_batch_step_async, rb_batch_*_dev; kernels in rb_batch_dev.hip)
// only enqueues and rb_batch_sync waits.
#include <cmath>

#include "rb_batch_contacts.hpp"
#include "rb_batch_dev.hpp"
#include "rb_batch_impulses.hpp"
#include "rb_batch_ragged.hpp"
#include "rb_host.hpp"
#include "rb_laneplan.hpp"
#include "rb_sampleplan.hpp"

using namespace rb::host;

static_assert(BATCH_EDOM == RB_EDOM && BATCH_CHUNK == RB_BATCH_CHUNK && BATCH_WIDE_MAX == RB_BATCH_MAX_BODIES, "batch constants");

struct rb_batch {
    int dtype = RB_F64, esz = 8, device = 0;
    hipStream_t stream = nullptr;      // where the batch's work is enqueued: own_stream, or the caller's
    hipStream_t own_stream = nullptr;  // created with the batch, destroyed with it
    int64_t E = 0, N = 0;              // environments, body slots (E * M)
    int32_t M = 0, n_planes = 0, oriented = 1;
    bool box = false;                  // the template is one box
    bool mixed = false;                // a box among several bodies (rb_batch_create_mixed): batch_mixed_kernel
    bool wide = false;                 // more than 64 bodies (rb_batch_create_wide): the kernels of rb_batch_wide.hip
    int32_t *d_kind = nullptr;         // [M] the template's kinds on the device (mixed)
    std::vector<int32_t> kind;         // [M] the template's kinds
    double planes[RB_MAX_PLANES][6] = {};
    double g[3] = {};
    double inv_cs = 1.0;
    void *snap = nullptr, *state = nullptr, *consts = nullptr;
    void *env_e = nullptr, *env_mu = nullptr;   // [E] reals; used while have_*
    bool have_e = false, have_mu = false;
    // per-environment planes [n_planes][6][E], gravity [3][E] and applied
    // forces [6][E * M] (reals; allocated by the first call that sets them,
    // used while have_*): any of them selects the ENVS step instances
    void *env_planes = nullptr, *env_g = nullptr, *env_xfrc = nullptr;
    bool have_planes = false, have_g = false, have_xfrc = false;
    int32_t *code = nullptr, *count = nullptr;
    int64_t *steps_done = nullptr;
    double *io_q = nullptr, *io_v = nullptr;    // device staging of the AoS rows
    int64_t io_rows = 0;
    int64_t *ids = nullptr;                     // device copy of an env_ids list
    int64_t ids_cap = 0;
    // contact law (rb_batch_set_contact_law)
    int32_t law = RB_LAW_MUJOCO;
    double tol = 0.01;
    double rmax = 0.0;                          // largest bounding radius
    // sampled runs (rb_batch_run_sampled): one allocation, first the sample
    // slots the recording kernels fill (the batch's real type), then the
    // boundary rows of as many samples (double), allocated on first use
    char *samp = nullptr;
    size_t samp_bytes = 0;                      // allocated
    size_t samp_limit = (size_t)256 << 20;      // RBHIP_BATCH_SAMPLE_BYTES
    // rb_batch_set_xfrc_dev: the smallest body slot an upload was refused for
    // (DEV_NO_SLOT: none), sticky until rb_batch_sync reports and clears it
    uint32_t *refused = nullptr;
    // rb_batch_contacts: device staging of the lists of a range of listed
    // environments (allocated on first use, it only grows, at most samp_limit bytes)
    char *con = nullptr;
    size_t con_bytes = 0;
    // the sizes last given (rb_batch_create, rb_batch_set_bodies): [E * M * 3];
    // a change of population derives the bounding radii from them again
    std::vector<double> size;
    // the population (rb_batch_set_population): while pop_set, the kernels of
    // rb_batch_ragged.hip step and query the batch
    bool pop_set = false;
    bool pop_boxes = false;            // a present body of some environment is a box
    bool pop_absent = false;           // some environment holds fewer than M bodies
    std::vector<int32_t> pop_n, pop_kind;       // [E], [E * M]
    int32_t *d_pop = nullptr;          // one allocation: n_bodies [E], kind [E * M], wave_env0 [waves + 1], lane_row [waves * 64]
    int32_t pop_waves = 0, pop_epw = 0;
};

namespace {

void free_batch(rb_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->own_stream) (void)hipStreamSynchronize(b->stream);
    void *bufs[] = {b->snap, b->state, b->consts, b->env_e, b->env_mu, b->code, b->count, b->steps_done,
                    b->io_q, b->io_v, b->ids, b->samp, b->env_planes, b->env_g, b->env_xfrc, b->d_kind, b->refused, b->con, b->d_pop};
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
    return b->pop_set ? b->pop_kind[(size_t)g] : b->kind[(size_t)(g % b->M)];
}
// is body slot g stepped (a present body)?
bool batch_present(const rb_batch *b, int64_t g) { return !b->pop_set || g % b->M < b->pop_n[(size_t)(g / b->M)]; }

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

template <typename T> BatchParams<T> batch_params(rb_batch *b, int32_t k, double dt, double e, double mu, double thr) {
    BatchParams<T> p{};
    p.snap = dp<Snap<T>>(b->snap, 0);
    p.st = BodyState<T>{dp<T>(b->state, 0), b->N};
    p.cs = BodyConsts<T>{dp<T>(b->consts, 0), b->N, b->d_kind};
    p.env_e = b->have_e ? dp<T>(b->env_e, 0) : nullptr;
    p.env_mu = b->have_mu ? dp<T>(b->env_mu, 0) : nullptr;
    p.code = b->code;
    p.steps_done = b->steps_done;
    p.E = b->E;
    p.M = b->M;
    p.k = k;
    p.n_planes = b->n_planes;
    p.oriented = b->oriented;
    for (int pl = 0; pl < b->n_planes; ++pl)
        for (int d = 0; d < 3; ++d) { p.pn[pl][d] = (T)b->planes[pl][d]; p.pp[pl][d] = (T)b->planes[pl][3 + d]; }
    for (int d = 0; d < 3; ++d) p.g[d] = (T)b->g[d];
    p.dt = (T)dt; p.e = (T)e; p.mu = (T)mu; p.thr = (T)thr;
    p.inv_cs = (T)b->inv_cs;
    p.tol = (T)b->tol;
    p.ground = b->n_planes == 1;
    p.env_planes = b->have_planes ? dp<T>(b->env_planes, 0) : nullptr;
    p.env_g = b->have_g ? dp<T>(b->env_g, 0) : nullptr;
    p.env_xfrc = b->have_xfrc ? dp<T>(b->env_xfrc, 0) : nullptr;
    return p;
}

// the population's device tables (b->d_pop)
Population batch_population(const rb_batch *b) {
    Population pop{};
    pop.n_bodies = b->d_pop;
    pop.kind = pop.n_bodies + b->E;
    if (!b->wide) {
        pop.wave_env0 = pop.kind + b->N;
        pop.lane_row = pop.wave_env0 + b->pop_waves + 1;
        pop.waves = b->pop_waves;
        pop.epw_max = b->pop_epw;
    }
    return pop;
}

// one launch of the batch's step kernel (rec: the recording instance)
template <typename T> hipError_t batch_launch(rb_batch *b, const BatchParams<T> &p, bool rec) {
    if (b->pop_set) return launch_ragged_step<T>(p, batch_population(b), b->pop_boxes, rec, b->stream);
    if (b->wide) return launch_batch_wide<T>(p, b->mixed, rec, b->stream);
    if (b->mixed) return launch_batch_mixed<T>(p, rec, b->stream);
    return launch_batch_step<T>(p, b->box, b->law == RB_LAW_BALLS, rec, b->stream);
}

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

// bytes one sample of the batch takes in the sample buffer: its slot (rounded
// up to whole doubles, so that the boundary rows behind the slots are aligned)
// and its boundary rows
size_t align8(size_t n) { return (n + 7) & ~(size_t)7; }
size_t sample_bytes(const rb_batch *b, int rows) {
    const size_t vals = (size_t)b->N * (size_t)rows;
    return align8(vals * (size_t)b->esz) + vals * sizeof(double);
}

// an env_ids list onto the device (b->ids)
int batch_put_ids(rb_batch *b, const int64_t *env_ids, int64_t n) {
    if (n > b->ids_cap) {
        if (b->ids) { HIPCHK(hipFree(b->ids)); b->ids = nullptr; }
        b->ids_cap = 0;
        HIPCHK(hipMalloc((void **)&b->ids, sizeof(int64_t) * (size_t)n));
        b->ids_cap = n;
    }
    HIPCHK(hipMemcpyAsync(b->ids, env_ids, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, b->stream));
    return RB_OK;
}

// the listed environments' rows: staging of n * M rows and the ids on the device
int batch_stage(rb_batch *b, const int64_t *env_ids, int64_t n) {
    const int64_t rows = n * b->M;
    if (rows > b->io_rows) {
        if (b->io_q) { HIPCHK(hipFree(b->io_q)); b->io_q = nullptr; }
        if (b->io_v) { HIPCHK(hipFree(b->io_v)); b->io_v = nullptr; }
        b->io_rows = 0;
        HIPCHK(hipMalloc((void **)&b->io_q, sizeof(double) * 7 * (size_t)rows));
        HIPCHK(hipMalloc((void **)&b->io_v, sizeof(double) * 6 * (size_t)rows));
        b->io_rows = rows;
    }
    if (env_ids) WCHK(batch_put_ids(b, env_ids, n));
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

// nsteps steps in launches of at most RB_BATCH_CHUNK steps: the state between
// two of them is the state between two steps, so the cut changes nothing
int batch_enqueue_steps(rb_batch *b, int64_t nsteps, double dt, double e, double mu, double thr) {
    for (int64_t left = nsteps; left > 0; left -= BATCH_CHUNK) {
        const int32_t k = (int32_t)std::min<int64_t>(left, BATCH_CHUNK);
        HIPCHK(by_real(b->dtype, [&](auto t) {
            using T = decltype(t);
            return batch_launch<T>(b, batch_params<T>(b, k, dt, e, mu, thr), false);
        }));
    }
    return RB_OK;
}

// launch l of a sampled run's plan, recording into the `fit` slots of `rows` rows at `slots`
int batch_enqueue_sampled(rb_batch *b, const SampleLaunch &l, char *slots, int64_t fit, int rows, int64_t every,
                          double dt, double e, double mu, double thr) {
    HIPCHK(by_real(b->dtype, [&](auto t) {
        using T = decltype(t);
        BatchParams<T> p = batch_params<T>(b, (int32_t)l.steps, dt, e, mu, thr);
        if (l.samples == 0)          // nothing to record in this launch: the plain instance
            return batch_launch<T>(b, p, false);
        p.samp = reinterpret_cast<T *>(slots);
        // phase and period travel as int32: a period past the chunk never samples
        // inside a launch that does not end on it, so it is clamped per launch
        p.every = (int32_t)std::min<int64_t>(every, BATCH_CHUNK + 1);   // (a second sample lies past the launch)
        p.phase = (int32_t)l.phase;                                     // (<= steps <= RB_BATCH_CHUNK here)
        p.samp_first = (int32_t)l.first;
        p.samp_slots = (int32_t)fit;
        p.samp_rows = rows;
        // absent bodies have no lane (or an idle one): their rows of the slots
        // this launch fills hold zeros
        if (b->pop_set && b->pop_absent) {
            const size_t slot = (size_t)b->N * (size_t)rows * sizeof(T);
            const hipError_t rc = hipMemsetAsync(slots + (size_t)l.first * slot, 0, (size_t)l.samples * slot, b->stream);
            if (rc != hipSuccess) return rc;
        }
        return batch_launch<T>(b, p, true);
    }));
    return RB_OK;
}

// the sample buffer for `fit` samples of `per` bytes each (it only grows)
int batch_sample_buffer(rb_batch *b, size_t per, int64_t fit) {
    const size_t need = per * (size_t)fit;
    if (need > b->samp_bytes) {
        if (b->samp) { HIPCHK(hipFree(b->samp)); b->samp = nullptr; }
        b->samp_bytes = 0;
        HIPCHK(hipMalloc((void **)&b->samp, need));
        b->samp_bytes = need;
    }
    return RB_OK;
}

// ---- the device-resident boundary ---------------------------------------------
template <typename T> DevState<T> batch_dev(rb_batch *b) {
    return DevState<T>{dp<Snap<T>>(b->snap, 0), BodyState<T>{dp<T>(b->state, 0), b->N}, dp<T>(b->consts, 7 * b->N),
                       b->code, b->steps_done, b->N, b->M};
}

int batch_check_io(int32_t io_dtype) {
    return io_dtype == RB_F64 || io_dtype == RB_F32 ? RB_OK : fail(RB_EINVAL, "io_dtype must be RB_F64 or RB_F32");
}

// a caller's array: device memory on the batch's device (a refusal leaves no HIP error behind)
int batch_dev_ptr(const rb_batch *b, const void *p, const char *name) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return fail(RB_EINVAL, "%s is not device memory (a host pointer?)", name);
    }
    if (a.device != b->device) return fail(RB_EINVAL, "%s is memory of device %d, the batch is on device %d", name, a.device, b->device);
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

// ---- the contact query (rb_batch_contacts, rb_batch_contacts_dev) ---------------
// the arguments both forms share, before any device call
int batch_check_contacts(const rb_batch *b, int32_t R, const void *counts, const void *partner, const void *kind,
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
int batch_check_contact_law(const rb_batch *b) {
    if (b->law == RB_LAW_BALLS)
        return fail(RB_EUNSUPPORTED, "the two-ball law has no contact list (its hit test carries a tolerance of its own)");
    return RB_OK;
}

// one launch of the query: rows [0, q.n) of q
int batch_launch_contacts(rb_batch *b, const ContactQuery &q) {
    HIPCHK(by_real(b->dtype, [&](auto t) {
        using T = decltype(t);
        const BatchParams<T> p = batch_params<T>(b, 0, 1.0, 0.0, 0.0, 0.0);
        if (b->pop_set) return launch_ragged_contacts<T>(p, batch_population(b), q, b->pop_boxes, b->stream);
        return b->wide ? launch_batch_wide_contacts<T>(p, q, b->mixed, b->stream)
                       : launch_batch_contacts<T>(p, q, b->mixed, b->stream);
    }));
    return RB_OK;
}

// ---- what the host forms of the queries share (rb_batch_contacts, rb_batch_impulses) ----
// the listed environments of a host form: n of them, in range, none twice
int batch_check_query_ids(const rb_batch *b, const int64_t *env_ids, int64_t n) {
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

// Does one listed environment (`per` bytes of `what`) fit the staging buffer?  (Before any device call.)
int batch_check_query_fit(const rb_batch *b, size_t per, const char *what) {
    if (per > b->samp_limit)
        return fail(RB_EINVAL, "%s of one environment (%zu bytes) do not fit the staging buffer (%zu bytes: "
                               "RBHIP_BATCH_SAMPLE_BYTES)", what, per, b->samp_limit);
    return RB_OK;
}

// The host form of a query over n >= 1 listed environments of `per` bytes each
// in the staging buffer (b->con; it only grows, at most samp_limit bytes): the
// ids onto the device, then a range of listed environments per launch.
// range(first, c) enqueues the launch and the downloads of the c environments
// from `first` on; the stream is waited for after each range, since the next
// one reuses the buffer.
template <typename F> int batch_query_ranges(rb_batch *b, const int64_t *env_ids, int64_t n, size_t per, F &&range) {
    const int64_t fit = std::min<int64_t>(n, (int64_t)(b->samp_limit / per));
    HIPCHK(hipSetDevice(b->device));
    if (per * (size_t)fit > b->con_bytes) {
        if (b->con) { HIPCHK(hipFree(b->con)); b->con = nullptr; }
        b->con_bytes = 0;
        HIPCHK(hipMalloc((void **)&b->con, per * (size_t)fit));
        b->con_bytes = per * (size_t)fit;
    }
    if (env_ids) WCHK(batch_put_ids(b, env_ids, n));
    for (int64_t first = 0; first < n; first += fit) {
        WCHK(range(first, (size_t)std::min<int64_t>(fit, n - first)));
        HIPCHK(hipStreamSynchronize(b->stream));
    }
    return RB_OK;
}

// a download of a range into the caller's array, on the batch's stream
hipError_t batch_get(rb_batch *b, void *dst, const void *src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, b->stream) : hipSuccess;
}

// the bodies whose true count is past R
int64_t batch_truncated(const int32_t *counts, size_t bodies, int32_t R) {
    int64_t t = 0;
    for (size_t k = 0; k < bodies; ++k) t += counts[k] > R;
    return t;
}

// every array of a device form that is given: device memory of the batch's device
int batch_dev_ptrs(const rb_batch *b, std::initializer_list<std::pair<const void *, const char *>> arrays) {
    for (const auto &a : arrays)
        if (a.first) WCHK(batch_dev_ptr(b, a.first, a.second));
    return RB_OK;
}

// ---- the impulse query (rb_batch_impulses, rb_batch_impulses_dev) ----------------
// the arguments both forms share, before any device call: the contact query's
// (jn and jt with the records), rb_batch_step's parameters, finite
int batch_check_impulses(const rb_batch *b, int32_t R, const void *counts, const void *partner, const void *kind,
                         const void *dist, const void *jn, const void *jt, double dt, double e, double mu, double thr) {
    WCHK(batch_check_contacts(b, R, counts, partner, kind, dist, nullptr, nullptr));
    if ((jn != nullptr) != (partner != nullptr) || (jt != nullptr) != (partner != nullptr))
        return fail(RB_EINVAL, "partner, kind, dist, jn and jt may be NULL only all together (max_records 0)");
    WCHK(batch_check_step(b, 1, dt, e, mu, thr));
    if (!std::isfinite(dt) || !std::isfinite(e) || !std::isfinite(mu) || !std::isfinite(thr))
        return fail(RB_EINVAL, "non-finite step parameters dt=%g e=%g mu=%g thr=%g", dt, e, mu, thr);
    return RB_OK;
}

// one launch of the query: rows [0, q.c.n) of q, by the batch's kind
int batch_launch_impulses(rb_batch *b, ImpulseQuery q, double dt, double e, double mu, double thr) {
    // (with a population the kinds are the population's: no one-box instance)
    q.c.box = b->box && !b->pop_set;
    HIPCHK(by_real(b->dtype, [&](auto t) {
        using T = decltype(t);
        const BatchParams<T> p = batch_params<T>(b, 1, dt, e, mu, thr);
        if (b->pop_set) return launch_batch_impulses<T>(p, batch_population(b), q, b->pop_boxes, b->stream);
        return launch_batch_impulses<T>(p, Population{}, q, b->mixed, b->stream);
    }));
    return RB_OK;
}

}  // namespace

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
    std::vector<int32_t> pn, pk;
    LanePlan plan;
    int32_t *tables = nullptr;
    bool boxes = false, absent = false;
    if (set) {
        if (n_bodies) pn.assign(n_bodies, n_bodies + b->E);
        else pn.assign((size_t)b->E, b->M);
        if (kind) pk.assign(kind, kind + b->N);
        else
            for (int64_t g = 0; g < b->N; ++g) pk.push_back(b->kind[(size_t)(g % b->M)]);
        for (int64_t g = 0; g < b->N; ++g) {
            const bool present = g % b->M < pn[(size_t)(g / b->M)];
            boxes = boxes || (present && pk[(size_t)g] == RB_BODY_BOX);
            absent = absent || !present;
        }
        std::vector<int32_t> h(pn);
        h.insert(h.end(), pk.begin(), pk.end());
        if (!b->wide) {
            if (!lane_plan(pn.data(), b->E, b->M, plan)) return fail(RB_EINVAL, "no lane plan for this population");
            h.insert(h.end(), plan.wave_env0.begin(), plan.wave_env0.end());
            h.insert(h.end(), plan.lane_row.begin(), plan.lane_row.end());
        }
        HIPCHK(hipMalloc((void **)&tables, sizeof(int32_t) * h.size()));
        if (int rc = bput(b, tables, h.data(), sizeof(int32_t) * h.size())) {
            (void)hipFree(tables);
            return rc;
        }
    }
    // commit; the bounding radii follow the kinds
    const bool was_set = b->pop_set, was_boxes = b->pop_boxes, was_absent = b->pop_absent;
    const int32_t was_waves = b->pop_waves, was_epw = b->pop_epw;
    const double was_rmax = b->rmax;
    b->pop_n.swap(pn);
    b->pop_kind.swap(pk);
    b->pop_set = set; b->pop_boxes = boxes; b->pop_absent = absent;
    b->pop_waves = plan.waves; b->pop_epw = plan.epw_max;
    if (int rc = batch_put_bounds(b)) {
        // (a device error; the host side is put back, and so are the radii, where the device still answers)
        b->pop_n.swap(pn);
        b->pop_kind.swap(pk);
        b->pop_set = was_set; b->pop_boxes = was_boxes; b->pop_absent = was_absent;
        b->pop_waves = was_waves; b->pop_epw = was_epw;
        b->rmax = was_rmax;
        (void)batch_put_bounds(b);
        if (tables) (void)hipFree(tables);
        return rc;
    }
    if (b->d_pop) (void)hipFree(b->d_pop);
    b->d_pop = tables;
    return RB_OK;
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
        if (b->pop_set)
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
    WCHK(batch_check_step(b, nsteps, dt, e, mu, thr));
    if (every < 1) return fail(RB_EINVAL, "every must be >= 1");
    const int64_t S = nsteps / every;
    if (S > 0 && !qpos) return fail(RB_EINVAL, "qpos NULL with %lld samples to record", (long long)S);
    HIPCHK(hipSetDevice(b->device));
    const int rows = qvel ? 13 : 7;
    const size_t per = sample_bytes(b, rows);
    int64_t fit = 1;
    if (S > 0) {
        if (per > b->samp_limit)
            return fail(RB_EINVAL, "one sample of the batch (%zu bytes) does not fit the sample buffer (%zu bytes: "
                                   "RBHIP_BATCH_SAMPLE_BYTES)", per, b->samp_limit);
        // no more slots than a launch index can address, than fit the bound, than the run needs
        fit = std::min<int64_t>({S, (int64_t)(b->samp_limit / per), (int64_t)INT32_MAX / 2});
        WCHK(batch_sample_buffer(b, per, fit));
    }
    // the slots first, the boundary rows of `fit` samples behind them
    const size_t N = (size_t)b->N;
    char *slots = b->samp;
    double *out_q = reinterpret_cast<double *>(b->samp + align8((size_t)fit * N * rows * b->esz));
    double *out_v = out_q + (size_t)fit * N * 7;

    SamplePlan plan(nsteps, every, BATCH_CHUNK, fit);
    SampleLaunch l;
    while (plan.next(l)) {
        WCHK(batch_enqueue_sampled(b, l, slots, fit, rows, every, dt, e, mu, thr));
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

// ---- the device-resident boundary: everything below but rb_batch_sync only enqueues ----

int rb_batch_set_stream(rb_batch *b, void *s) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    HIPCHK(hipSetDevice(b->device));
    // work queued on the old stream finishes there before later work is ordered on the new one
    HIPCHK(hipStreamSynchronize(b->stream));
    b->stream = (hipStream_t)s;        // NULL = HIP's null stream
    return RB_OK;
}

int rb_batch_step_async(rb_batch *b, int64_t nsteps, double dt, double e, double mu, double thr) {
    ApiScope api_scope_(b ? b->device : -1);
    WCHK(batch_check_step(b, nsteps, dt, e, mu, thr));
    HIPCHK(hipSetDevice(b->device));
    return batch_enqueue_steps(b, nsteps, dt, e, mu, thr);
}

int rb_batch_sync(rb_batch *b, int64_t *n_failed) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    HIPCHK(hipSetDevice(b->device));
    // the refusal word of rb_batch_set_xfrc_dev: read and cleared, in stream order
    uint32_t slot = DEV_NO_SLOT;
    HIPCHK(hipMemcpyAsync(&slot, b->refused, sizeof(slot), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipMemsetAsync(b->refused, 0xff, sizeof(slot), b->stream));
    const int rc = batch_report(b, n_failed);      // (waits for the stream)
    if (rc != RB_OK && rc != RB_EDOM) return rc;
    if (slot != DEV_NO_SLOT)
        return fail(RB_EINVAL, "rb_batch_set_xfrc_dev: environment %lld, body %lld: non-finite applied force or torque "
                               "(that upload and every later one up to this call wrote nothing)",
                    (long long)(slot / (uint32_t)b->M), (long long)(slot % (uint32_t)b->M));
    return rc;
}

int rb_batch_set_state_dev(rb_batch *b, const uint8_t *mask, const void *qpos, const void *qvel, int32_t io_dtype) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    if (!qpos || !qvel) return fail(RB_EINVAL, "null argument");
    WCHK(batch_check_io(io_dtype));
    HIPCHK(hipSetDevice(b->device));
    if (mask) WCHK(batch_dev_ptr(b, mask, "mask"));
    WCHK(batch_dev_ptr(b, qpos, "qpos"));
    WCHK(batch_dev_ptr(b, qvel, "qvel"));
    HIPCHK(by_real(b->dtype, [&](auto t) {
        using T = decltype(t);
        return by_real(io_dtype, [&](auto io) {
            using IO = decltype(io);
            return launch_dev_state_in<T, IO>(batch_dev<T>(b), mask, (const IO *)qpos, (const IO *)qvel, b->stream);
        });
    }));
    return RB_OK;
}

int rb_batch_get_state_dev(rb_batch *b, void *qpos, void *qvel, int32_t io_dtype) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    if (!qpos && !qvel) return fail(RB_EINVAL, "null argument");
    WCHK(batch_check_io(io_dtype));
    HIPCHK(hipSetDevice(b->device));
    if (qpos) WCHK(batch_dev_ptr(b, qpos, "qpos"));
    if (qvel) WCHK(batch_dev_ptr(b, qvel, "qvel"));
    HIPCHK(by_real(b->dtype, [&](auto t) {
        using T = decltype(t);
        return by_real(io_dtype, [&](auto io) {
            using IO = decltype(io);
            return launch_dev_state_out<T, IO>(batch_dev<T>(b), (IO *)qpos, (IO *)qvel, b->stream);
        });
    }));
    return RB_OK;
}

int rb_batch_set_xfrc_dev(rb_batch *b, const void *xfrc, int32_t io_dtype) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    if (!xfrc) return fail(RB_EINVAL, "xfrc NULL (rb_batch_set_xfrc(b, NULL) clears the applied forces)");
    WCHK(batch_check_io(io_dtype));
    if (b->law == RB_LAW_BALLS)
        return fail(RB_EUNSUPPORTED, "the two-ball law takes no applied forces (ball_collision.py:73-125)");
    HIPCHK(hipSetDevice(b->device));
    WCHK(batch_dev_ptr(b, xfrc, "xfrc"));
    if (!b->env_xfrc) {
        const size_t bytes = (size_t)b->N * 6 * (size_t)b->esz;
        void *rows = nullptr;
        HIPCHK(hipMalloc(&rows, bytes));
        b->env_xfrc = rows;
        HIPCHK(hipMemsetAsync(rows, 0, bytes, b->stream));
    }
    // the host cannot see the check's outcome: forces count as set from here on
    b->have_xfrc = true;
    HIPCHK(by_real(io_dtype, [&](auto io) {
        using IO = decltype(io);
        return launch_dev_xfrc_check<IO>((const IO *)xfrc, b->N, b->refused, b->stream);
    }));
    HIPCHK(by_real(b->dtype, [&](auto t) {
        using T = decltype(t);
        return by_real(io_dtype, [&](auto io) {
            using IO = decltype(io);
            return launch_dev_xfrc_in<T, IO>((const IO *)xfrc, dp<T>(b->env_xfrc, 0), b->N, b->refused, b->stream);
        });
    }));
    return RB_OK;
}

int rb_batch_status_dev(rb_batch *b, int32_t *code, int64_t *steps_done) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    if (!code && !steps_done) return fail(RB_EINVAL, "null argument");
    HIPCHK(hipSetDevice(b->device));
    if (code) WCHK(batch_dev_ptr(b, code, "code"));
    if (steps_done) WCHK(batch_dev_ptr(b, steps_done, "steps_done"));
    if (code) HIPCHK(hipMemcpyAsync(code, b->code, sizeof(int32_t) * (size_t)b->E, hipMemcpyDeviceToDevice, b->stream));
    if (steps_done)
        HIPCHK(hipMemcpyAsync(steps_done, b->steps_done, sizeof(int64_t) * (size_t)b->E, hipMemcpyDeviceToDevice, b->stream));
    return RB_OK;
}

int rb_batch_run_sampled_dev(rb_batch *b, int64_t nsteps, int64_t every, double dt, double e, double mu, double thr,
                             void *qpos, void *qvel, int32_t io_dtype) {
    ApiScope api_scope_(b ? b->device : -1);
    WCHK(batch_check_step(b, nsteps, dt, e, mu, thr));
    if (every < 1) return fail(RB_EINVAL, "every must be >= 1");
    WCHK(batch_check_io(io_dtype));
    const int64_t S = nsteps / every;
    if (S > 0 && !qpos) return fail(RB_EINVAL, "qpos NULL with %lld samples to record", (long long)S);
    HIPCHK(hipSetDevice(b->device));
    const int rows = qvel ? 13 : 7;
    // the buffer holds the slots alone: the drain writes the caller's arrays
    const size_t per = (size_t)b->N * (size_t)rows * (size_t)b->esz;
    int64_t fit = 1;
    if (S > 0) {
        WCHK(batch_dev_ptr(b, qpos, "qpos"));
        if (qvel) WCHK(batch_dev_ptr(b, qvel, "qvel"));
        if (per > b->samp_limit)
            return fail(RB_EINVAL, "one sample of the batch (%zu bytes) does not fit the sample buffer (%zu bytes: "
                                   "RBHIP_BATCH_SAMPLE_BYTES)", per, b->samp_limit);
        fit = std::min<int64_t>({S, (int64_t)(b->samp_limit / per), (int64_t)INT32_MAX / 2});
        WCHK(batch_sample_buffer(b, per, fit));
    }
    const size_t N = (size_t)b->N;
    SamplePlan plan(nsteps, every, BATCH_CHUNK, fit);
    SampleLaunch l;
    while (plan.next(l)) {
        WCHK(batch_enqueue_sampled(b, l, b->samp, fit, rows, every, dt, e, mu, thr));
        if (l.drain == 0) continue;
        // the drain: one transpose from the slots into the caller's arrays, in stream order
        const size_t at = (size_t)l.drain_at * N;
        HIPCHK(by_real(b->dtype, [&](auto t) {
            using T = decltype(t);
            return by_real(io_dtype, [&](auto io) {
                using IO = decltype(io);
                return launch_dev_samples_out<T, IO>(reinterpret_cast<const T *>(b->samp), (int32_t)l.drain, rows, b->N,
                                                     (IO *)qpos + 7 * at, qvel ? (IO *)qvel + 6 * at : nullptr, b->stream);
            });
        }));
    }
    return RB_OK;
}

// ---- the contact query ----------------------------------------------------------

int rb_batch_contacts(rb_batch *b, const int64_t *env_ids, int64_t n, int32_t max_records, int32_t *counts,
                      int32_t *partner, int32_t *kind, double *dist, double *pos, double *frame, int64_t *n_truncated) {
    ApiScope api_scope_(b ? b->device : -1);
    const int32_t R = max_records;
    WCHK(batch_check_contacts(b, R, counts, partner, kind, dist, pos, frame));
    WCHK(batch_check_query_ids(b, env_ids, n));
    WCHK(batch_check_contact_law(b));
    if (n_truncated) *n_truncated = 0;
    if (n == 0) return RB_OK;
    // one listed environment in the staging buffer: the reals first (aligned), then the words
    const size_t M = (size_t)b->M, MR = M * (size_t)R;
    const size_t per = sizeof(double) * MR * (1 + (pos ? 3 : 0) + (frame ? 3 : 0)) + sizeof(int32_t) * (M + 2 * MR);
    WCHK(batch_check_query_fit(b, per, "the contact lists"));
    WCHK(batch_query_ranges(b, env_ids, n, per, [&](int64_t first, size_t c) {
        const size_t at = (size_t)first;
        double *d_dist = reinterpret_cast<double *>(b->con);
        double *d_pos = d_dist + c * MR, *d_frame = d_pos + (pos ? 3 * c * MR : 0);
        int32_t *d_counts = reinterpret_cast<int32_t *>(d_frame + (frame ? 3 * c * MR : 0));
        int32_t *d_partner = d_counts + c * M, *d_kind = d_partner + c * MR;
        ContactQuery q{};
        q.counts = d_counts;
        if (R > 0) { q.partner = d_partner; q.kind = d_kind; q.dist = d_dist; }
        q.pos = pos ? d_pos : nullptr;
        q.frame = frame ? d_frame : nullptr;
        q.ids = env_ids ? b->ids + first : nullptr;
        q.env0 = first;
        q.n = (int64_t)c;
        q.R = R;
        q.io32 = 0;
        q.box = b->box;
        WCHK(batch_launch_contacts(b, q));
        HIPCHK(batch_get(b, counts + at * M, d_counts, sizeof(int32_t) * c * M));
        if (R > 0) {
            HIPCHK(batch_get(b, partner + at * MR, d_partner, sizeof(int32_t) * c * MR));
            HIPCHK(batch_get(b, kind + at * MR, d_kind, sizeof(int32_t) * c * MR));
            HIPCHK(batch_get(b, dist + at * MR, d_dist, sizeof(double) * c * MR));
            if (pos) HIPCHK(batch_get(b, pos + 3 * at * MR, d_pos, sizeof(double) * 3 * c * MR));
            if (frame) HIPCHK(batch_get(b, frame + 3 * at * MR, d_frame, sizeof(double) * 3 * c * MR));
        }
        return (int)RB_OK;
    }));
    if (n_truncated) *n_truncated = batch_truncated(counts, (size_t)n * M, R);
    return RB_OK;
}

int rb_batch_contacts_dev(rb_batch *b, int32_t max_records, int32_t *counts, int32_t *partner, int32_t *kind,
                          void *dist, void *pos, void *frame, int32_t io_dtype) {
    ApiScope api_scope_(b ? b->device : -1);
    WCHK(batch_check_contacts(b, max_records, counts, partner, kind, dist, pos, frame));
    WCHK(batch_check_io(io_dtype));
    WCHK(batch_check_contact_law(b));
    HIPCHK(hipSetDevice(b->device));
    WCHK(batch_dev_ptrs(b, {{counts, "counts"}, {partner, "partner"}, {kind, "kind"}, {dist, "dist"}, {pos, "pos"}, {frame, "frame"}}));
    ContactQuery q{};
    q.counts = counts;
    q.partner = partner;
    q.kind = kind;
    q.dist = dist;
    q.pos = pos;
    q.frame = frame;
    q.n = b->E;
    q.R = max_records;
    q.io32 = io_dtype == RB_F32;
    q.box = b->box;
    return batch_launch_contacts(b, q);
}

// ---- the impulse query ----------------------------------------------------------

int rb_batch_impulses(rb_batch *b, const int64_t *env_ids, int64_t n, int32_t max_records, double dt, double restitution,
                      double friction, double contact_threshold, int32_t *counts, int32_t *partner, int32_t *kind,
                      double *dist, double *jn, double *jt, double *vel, double *net, int64_t *n_truncated) {
    ApiScope api_scope_(b ? b->device : -1);
    const int32_t R = max_records;
    WCHK(batch_check_impulses(b, R, counts, partner, kind, dist, jn, jt, dt, restitution, friction, contact_threshold));
    WCHK(batch_check_query_ids(b, env_ids, n));
    WCHK(batch_check_contact_law(b));
    if (n_truncated) *n_truncated = 0;
    if (n == 0) return RB_OK;
    // one listed environment in the staging buffer: the reals first (aligned), then the words
    const size_t M = (size_t)b->M, MR = M * (size_t)R;
    const size_t per = sizeof(double) * (5 * MR + (vel ? 6 * M : 0) + (net ? 6 * M : 0)) + sizeof(int32_t) * (M + 2 * MR);
    WCHK(batch_check_query_fit(b, per, "the impulse records"));
    WCHK(batch_query_ranges(b, env_ids, n, per, [&](int64_t first, size_t c) {
        const size_t at = (size_t)first;
        double *d_dist = reinterpret_cast<double *>(b->con);
        double *d_jn = d_dist + c * MR, *d_jt = d_jn + c * MR, *d_vel = d_jt + 3 * c * MR;
        double *d_net = d_vel + (vel ? 6 * c * M : 0);
        int32_t *d_counts = reinterpret_cast<int32_t *>(d_net + (net ? 6 * c * M : 0));
        int32_t *d_partner = d_counts + c * M, *d_kind = d_partner + c * MR;
        ImpulseQuery q{};
        q.c.counts = d_counts;
        if (R > 0) { q.c.partner = d_partner; q.c.kind = d_kind; q.c.dist = d_dist; q.jn = d_jn; q.jt = d_jt; }
        q.vel = vel ? d_vel : nullptr;
        q.net = net ? d_net : nullptr;
        q.c.ids = env_ids ? b->ids + first : nullptr;
        q.c.env0 = first;
        q.c.n = (int64_t)c;
        q.c.R = R;
        q.c.io32 = 0;
        WCHK(batch_launch_impulses(b, q, dt, restitution, friction, contact_threshold));
        HIPCHK(batch_get(b, counts + at * M, d_counts, sizeof(int32_t) * c * M));
        if (R > 0) {
            HIPCHK(batch_get(b, partner + at * MR, d_partner, sizeof(int32_t) * c * MR));
            HIPCHK(batch_get(b, kind + at * MR, d_kind, sizeof(int32_t) * c * MR));
            HIPCHK(batch_get(b, dist + at * MR, d_dist, sizeof(double) * c * MR));
            HIPCHK(batch_get(b, jn + at * MR, d_jn, sizeof(double) * c * MR));
            HIPCHK(batch_get(b, jt + 3 * at * MR, d_jt, sizeof(double) * 3 * c * MR));
        }
        if (vel) HIPCHK(batch_get(b, vel + 6 * at * M, d_vel, sizeof(double) * 6 * c * M));
        if (net) HIPCHK(batch_get(b, net + 6 * at * M, d_net, sizeof(double) * 6 * c * M));
        return (int)RB_OK;
    }));
    if (n_truncated) *n_truncated = batch_truncated(counts, (size_t)n * M, R);
    return RB_OK;
}

int rb_batch_impulses_dev(rb_batch *b, int32_t max_records, double dt, double restitution, double friction,
                          double contact_threshold, int32_t *counts, int32_t *partner, int32_t *kind, void *dist, void *jn,
                          void *jt, void *vel, void *net, int32_t io_dtype) {
    ApiScope api_scope_(b ? b->device : -1);
    WCHK(batch_check_impulses(b, max_records, counts, partner, kind, dist, jn, jt, dt, restitution, friction,
                              contact_threshold));
    WCHK(batch_check_io(io_dtype));
    WCHK(batch_check_contact_law(b));
    HIPCHK(hipSetDevice(b->device));
    WCHK(batch_dev_ptrs(b, {{counts, "counts"}, {partner, "partner"}, {kind, "kind"}, {dist, "dist"}, {jn, "jn"}, {jt, "jt"},
                            {vel, "vel"}, {net, "net"}}));
    ImpulseQuery q{};
    q.c.counts = counts;
    q.c.partner = partner;
    q.c.kind = kind;
    q.c.dist = dist;
    q.jn = jn;
    q.jt = jt;
    q.vel = vel;
    q.net = net;
    q.c.n = b->E;
    q.c.R = max_records;
    q.c.io32 = io_dtype == RB_F32;
    return batch_launch_impulses(b, q, dt, restitution, friction, contact_threshold);
}

}  // extern "C"
