// rb_api_batch_dev.hip — the enqueue side of a batch.  First what every launch
// shares: the kernels' argument block (batch_params), the step launches
// (batch_enqueue_steps) and a sampled run's prelude and launches (with them
// those of a run that records impulse curves: batch_sensed_prelude,
// batch_enqueue_sensed), which rb_batch_step, rb_batch_run_sampled and
// rb_batch_run_sampled_impulses wait for and the entries here do not.
// Then the device-resident boundary (rb_batch_set_stream, rb_batch_step_async,
// rb_batch_sync, rb_batch_*_dev but the queries'; kernels in rb_batch_dev.hip):
// the caller's arrays are device memory on the batch's device, every entry but
// rb_batch_sync only enqueues on the batch's stream, and rb_batch_sync waits
// and reports.
#include "rb_batch_dev.hpp"
#include "rb_batch_host.hpp"

namespace rb::host {

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
template BatchParams<double> batch_params<double>(rb_batch *, int32_t, double, double, double, double);
template BatchParams<float> batch_params<float>(rb_batch *, int32_t, double, double, double, double);

// the population's device tables (b->pop.tables)
Population batch_population(const rb_batch *b) {
    Population pop{};
    pop.n_bodies = b->pop.tables;
    pop.kind = pop.n_bodies + b->E;
    if (!b->wide) {
        pop.wave_env0 = pop.kind + b->N;
        pop.lane_row = pop.wave_env0 + b->pop.waves + 1;
        pop.waves = b->pop.waves;
        pop.epw_max = b->pop.epw;
    }
    return pop;
}

// one launch of the batch's step kernel (rec: the recording instance)
template <typename T> static hipError_t batch_launch(rb_batch *b, const BatchParams<T> &p, bool rec) {
    if (b->pop.set) return launch_ragged_step<T>(p, batch_population(b), b->pop.boxes, rec, b->stream);
    if (b->wide) return launch_batch_wide<T>(p, b->mixed, rec, b->stream);
    if (b->mixed) return launch_batch_mixed<T>(p, rec, b->stream);
    return launch_batch_step<T>(p, b->box, b->law == RB_LAW_BALLS, rec, b->stream);
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

int batch_sampled_prelude(rb_batch *b, int64_t nsteps, int64_t every, double dt, double e, double mu, double thr,
                          const void *qpos, const void *qvel, const int32_t *io_dtype,
                          size_t (*per)(const rb_batch *, int rows), SampledRun &r) {
    WCHK(batch_check_step(b, nsteps, dt, e, mu, thr));
    if (every < 1) return fail(RB_EINVAL, "every must be >= 1");
    if (io_dtype) WCHK(batch_check_io(*io_dtype));
    const int64_t S = nsteps / every;
    if (S > 0 && !qpos) return fail(RB_EINVAL, "qpos NULL with %lld samples to record", (long long)S);
    HIPCHK(hipSetDevice(b->device));
    r.rows = qvel ? 13 : 7;
    r.fit = 1;
    if (S == 0) return RB_OK;
    if (io_dtype) WCHK(dev_ptrs(b->device, "batch", {{qpos, "qpos"}, {qvel, "qvel"}}));
    const size_t bytes = per(b, r.rows);
    if (bytes > b->samp_limit)
        return fail(RB_EINVAL, "one sample of the batch (%zu bytes) does not fit the sample buffer (%zu bytes: "
                               "RBHIP_BATCH_SAMPLE_BYTES)", bytes, b->samp_limit);
    // no more slots than a launch index can address, than fit the bound, than the run needs
    r.fit = std::min<int64_t>({S, (int64_t)(b->samp_limit / bytes), (int64_t)INT32_MAX / 2});
    return grow((void **)&b->samp, &b->samp_bytes, bytes * (size_t)r.fit);
}

int batch_enqueue_sampled(rb_batch *b, const SampleLaunch &l, char *slots, const SampledRun &r, int64_t every, double dt,
                          double e, double mu, double thr) {
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
        p.samp_slots = (int32_t)r.fit;
        p.samp_rows = r.rows;
        // absent bodies have no lane (or an idle one): their rows of the slots
        // this launch fills hold zeros
        if (b->pop.set && b->pop.absent) {
            const size_t slot = (size_t)b->N * (size_t)r.rows * sizeof(T);
            const hipError_t rc = hipMemsetAsync(slots + (size_t)l.first * slot, 0, (size_t)l.samples * slot, b->stream);
            if (rc != hipSuccess) return rc;
        }
        return batch_launch<T>(b, p, true);
    }));
    return RB_OK;
}

int batch_sensed_prelude(rb_batch *b, int64_t nsteps, int64_t every, double dt, double e, double mu, double thr,
                         const void *qpos, const void *qvel, const void *net, const int32_t *io_dtype,
                         size_t (*per)(const rb_batch *, int rows), SampledRun &r) {
    WCHK(batch_check_step(b, nsteps, dt, e, mu, thr));
    if (every < 1) return fail(RB_EINVAL, "every must be >= 1");
    if (io_dtype) WCHK(batch_check_io(*io_dtype));
    if (b->law == RB_LAW_BALLS)
        return fail(RB_EUNSUPPORTED, "the two-ball law records no impulse curves (it has no contact list: rb_batch_impulses)");
    const int64_t S = nsteps / every;
    if (S > 0 && !net) return fail(RB_EINVAL, "net NULL with %lld samples to record", (long long)S);
    HIPCHK(hipSetDevice(b->device));
    r.rows = sensed_rows(qpos != nullptr, qvel != nullptr);
    r.fit = 1;
    if (S == 0) return RB_OK;
    if (io_dtype) WCHK(dev_ptrs(b->device, "batch", {{qpos, "qpos"}, {qvel, "qvel"}, {net, "net"}}));
    const size_t bytes = per(b, r.rows);
    if (bytes > b->samp_limit)
        return fail(RB_EINVAL, "one sample of the batch (%zu bytes) does not fit the sample buffer (%zu bytes: "
                               "RBHIP_BATCH_SAMPLE_BYTES)", bytes, b->samp_limit);
    r.fit = std::min<int64_t>({S, (int64_t)(b->samp_limit / bytes), (int64_t)INT32_MAX / 2});
    WCHK(grow((void **)&b->samp, &b->samp_bytes, bytes * (size_t)r.fit));
    return grow(&b->sense, &b->sense_bytes, (size_t)b->N * 6 * (size_t)b->esz);
}

SensedRun batch_sensed_run(const rb_batch *b, bool want_q, bool want_v) {
    // (with a population the kinds are the population's: no one-box instance)
    return sensed_run(b->sense, b->box && !b->pop.set, want_q, want_v);
}

int batch_enqueue_sensed(rb_batch *b, const SampleLaunch &l, char *slots, const SampledRun &r, const SensedRun &sr,
                         int64_t every, double dt, double e, double mu, double thr) {
    HIPCHK(by_real(b->dtype, [&](auto t) {
        using T = decltype(t);
        BatchParams<T> p = batch_params<T>(b, (int32_t)l.steps, dt, e, mu, thr);
        p.samp = reinterpret_cast<T *>(slots);
        // phase and period travel as int32, clamped per launch as batch_enqueue_sampled clamps them; a
        // launch without a sample (its phase lies past its steps) senses all the same: the window runs on
        p.every = (int32_t)std::min<int64_t>(every, BATCH_CHUNK + 1);
        p.phase = (int32_t)std::min<int64_t>(l.phase, BATCH_CHUNK + 1);
        p.samp_first = (int32_t)l.first;
        p.samp_slots = (int32_t)r.fit;
        p.samp_rows = r.rows;
        // absent bodies store nothing: their rows of the slots this launch fills hold zeros
        if (b->pop.set && b->pop.absent && l.samples > 0) {
            const size_t slot = (size_t)b->N * (size_t)r.rows * sizeof(T);
            const hipError_t rc = hipMemsetAsync(slots + (size_t)l.first * slot, 0, (size_t)l.samples * slot, b->stream);
            if (rc != hipSuccess) return rc;
        }
        if (b->pop.set) return launch_batch_sensed<T>(p, batch_population(b), sr, b->pop.boxes, b->stream);
        return launch_batch_sensed<T>(p, Population{}, sr, b->mixed, b->stream);
    }));
    return RB_OK;
}

int batch_check_io(int32_t io_dtype) {
    return io_dtype == RB_F64 || io_dtype == RB_F32 ? RB_OK : fail(RB_EINVAL, "io_dtype must be RB_F64 or RB_F32");
}

// f(T{}, IO{}): T the batch's real type, IO the caller's element type
template <typename F> static auto by_real_io(const rb_batch *b, int32_t io_dtype, F &&f) {
    return by_real(b->dtype, [&](auto t) { return by_real(io_dtype, [&](auto io) { return f(t, io); }); });
}

template <typename T> static DevState<T> batch_dev(rb_batch *b) {
    return DevState<T>{dp<Snap<T>>(b->snap, 0), BodyState<T>{dp<T>(b->state, 0), b->N}, dp<T>(b->consts, 7 * b->N),
                       b->code, b->steps_done, b->N, b->M};
}

// a sample of the device form: its slot alone (the drain writes the caller's arrays)
static size_t slot_bytes(const rb_batch *b, int rows) { return (size_t)b->N * (size_t)rows * (size_t)b->esz; }

}  // namespace rb::host

using namespace rb::host;

extern "C" {

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
    WCHK(dev_ptrs(b->device, "batch", {{mask, "mask"}, {qpos, "qpos"}, {qvel, "qvel"}}));
    HIPCHK(by_real_io(b, io_dtype, [&](auto t, auto io) {
        using T = decltype(t);
        using IO = decltype(io);
        return launch_dev_state_in<T, IO>(batch_dev<T>(b), mask, (const IO *)qpos, (const IO *)qvel, b->stream);
    }));
    return RB_OK;
}

int rb_batch_get_state_dev(rb_batch *b, void *qpos, void *qvel, int32_t io_dtype) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    if (!qpos && !qvel) return fail(RB_EINVAL, "null argument");
    WCHK(batch_check_io(io_dtype));
    HIPCHK(hipSetDevice(b->device));
    WCHK(dev_ptrs(b->device, "batch", {{qpos, "qpos"}, {qvel, "qvel"}}));
    HIPCHK(by_real_io(b, io_dtype, [&](auto t, auto io) {
        using T = decltype(t);
        using IO = decltype(io);
        return launch_dev_state_out<T, IO>(batch_dev<T>(b), (IO *)qpos, (IO *)qvel, b->stream);
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
    WCHK(dev_ptrs(b->device, "batch", {{xfrc, "xfrc"}}));
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
    HIPCHK(by_real_io(b, io_dtype, [&](auto t, auto io) {
        using T = decltype(t);
        using IO = decltype(io);
        return launch_dev_xfrc_in<T, IO>((const IO *)xfrc, dp<T>(b->env_xfrc, 0), b->N, b->refused, b->stream);
    }));
    return RB_OK;
}

int rb_batch_status_dev(rb_batch *b, int32_t *code, int64_t *steps_done) {
    ApiScope api_scope_(b ? b->device : -1);
    if (!b) return fail(RB_EINVAL, "null batch");
    if (!code && !steps_done) return fail(RB_EINVAL, "null argument");
    HIPCHK(hipSetDevice(b->device));
    WCHK(dev_ptrs(b->device, "batch", {{code, "code"}, {steps_done, "steps_done"}}));
    if (code) HIPCHK(hipMemcpyAsync(code, b->code, sizeof(int32_t) * (size_t)b->E, hipMemcpyDeviceToDevice, b->stream));
    if (steps_done)
        HIPCHK(hipMemcpyAsync(steps_done, b->steps_done, sizeof(int64_t) * (size_t)b->E, hipMemcpyDeviceToDevice, b->stream));
    return RB_OK;
}

int rb_batch_run_sampled_dev(rb_batch *b, int64_t nsteps, int64_t every, double dt, double e, double mu, double thr,
                             void *qpos, void *qvel, int32_t io_dtype) {
    ApiScope api_scope_(b ? b->device : -1);
    SampledRun r;
    WCHK(batch_sampled_prelude(b, nsteps, every, dt, e, mu, thr, qpos, qvel, &io_dtype, slot_bytes, r));
    const size_t N = (size_t)b->N;
    SamplePlan plan(nsteps, every, BATCH_CHUNK, r.fit);
    SampleLaunch l;
    while (plan.next(l)) {
        WCHK(batch_enqueue_sampled(b, l, b->samp, r, every, dt, e, mu, thr));
        if (l.drain == 0) continue;
        // the drain: one transpose from the slots into the caller's arrays, in stream order
        const size_t at = (size_t)l.drain_at * N;
        HIPCHK(by_real_io(b, io_dtype, [&](auto t, auto io) {
            using T = decltype(t);
            using IO = decltype(io);
            return launch_dev_samples_out<T, IO>(reinterpret_cast<const T *>(b->samp), (int32_t)l.drain, r.rows, b->N,
                                                 (IO *)qpos + 7 * at, qvel ? (IO *)qvel + 6 * at : nullptr, b->stream);
        }));
    }
    return RB_OK;
}

int rb_batch_run_sampled_impulses_dev(rb_batch *b, int64_t nsteps, int64_t every, double dt, double e, double mu,
                                      double thr, void *qpos, void *qvel, void *net, int32_t io_dtype) {
    ApiScope api_scope_(b ? b->device : -1);
    SampledRun r;
    WCHK(batch_sensed_prelude(b, nsteps, every, dt, e, mu, thr, qpos, qvel, net, &io_dtype, slot_bytes, r));
    if (nsteps / every == 0) return batch_enqueue_steps(b, nsteps, dt, e, mu, thr);   // no window: nothing to sense
    const size_t N = (size_t)b->N;
    const SensedRun sr = batch_sensed_run(b, qpos != nullptr, qvel != nullptr);
    HIPCHK(hipMemsetAsync(b->sense, 0, N * 6 * (size_t)b->esz, b->stream));           // the first window starts from +0
    SamplePlan plan(nsteps, every, BATCH_CHUNK, r.fit);
    SampleLaunch l;
    while (plan.next(l)) {
        WCHK(batch_enqueue_sensed(b, l, b->samp, r, sr, every, dt, e, mu, thr));
        if (l.drain == 0) continue;
        const size_t at = (size_t)l.drain_at * N;
        HIPCHK(by_real_io(b, io_dtype, [&](auto t, auto io) {
            using T = decltype(t);
            using IO = decltype(io);
            return launch_sensed_out<T, IO>(reinterpret_cast<const T *>(b->samp), (int32_t)l.drain, r.rows, sr, b->N,
                                            qpos ? (IO *)qpos + 7 * at : nullptr, qvel ? (IO *)qvel + 6 * at : nullptr,
                                            (IO *)net + 6 * at, b->stream);
        }));
    }
    return RB_OK;
}

}  // extern "C"
