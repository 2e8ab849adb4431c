// rb_api_guard.hip — guarded chunks: the chunk-start copy, the check after
// the chunk and the roll-back; what a roll-back changes before the replay
// (the table grown, max_partners raised, the layout's period refitted).
#include "rb_host.hpp"

namespace rb::host {

// Guarded chunks (enqueue_steps): the chunk-start copy (state rows,
// snapshot, box orientations, error word), the check after the chunk (error
// word, deferral counts: one host sync), the roll-back.
static size_t chunk_save_bytes(const rb_world *w) {
    return state_bytes(w) + 2 * snap_bytes(w) + sizeof(int32_t);
}
static int chunk_save(rb_world *w) {
    if (!w->opt_save) {
        WCHK(w->opt_save.alloc(chunk_save_bytes(w)));
        WCHK(w->defer_host.alloc(sizeof(int32_t) * 4));
    }
    char *o = static_cast<char *>(w->opt_save.get());
    const size_t st = state_bytes(w), sn = snap_bytes(w);
    HIPCHK(hipMemcpyAsync(o, w->state, st, hipMemcpyDeviceToDevice, w->stream));
    HIPCHK(hipMemcpyAsync(o + st, w->snap[w->sp()], sn, hipMemcpyDeviceToDevice, w->stream));
    if (w->boxes) HIPCHK(hipMemcpyAsync(o + st + sn, w->qsnap[w->sp()], sn, hipMemcpyDeviceToDevice, w->stream));
    HIPCHK(hipMemcpyAsync(o + st + 2 * sn, w->err, sizeof(int32_t), hipMemcpyDeviceToDevice, w->stream));
    // the error bits from before the chunk (an earlier rb_step_async), read with the check
    HIPCHK(hipMemcpyAsync(w->defer_host + 3, w->err, sizeof(int32_t), hipMemcpyDeviceToHost, w->stream));
    if (w->boxes) HIPCHK(hipMemsetAsync(w->defer_cnt, 0, sizeof(int32_t) * 2, w->stream));
    return RB_OK;
}
static int chunk_check(rb_world *w, int32_t &err, bool &deferred) {
    HIPCHK(hipMemcpyAsync(w->defer_host, w->err, sizeof(int32_t), hipMemcpyDeviceToHost, w->stream));
    if (w->boxes) HIPCHK(hipMemcpyAsync(w->defer_host + 1, w->defer_cnt, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    err = w->defer_host[0] & ~w->defer_host[3];       // raised during this chunk
    if (w->diag_overflow > 0) { --w->diag_overflow; err |= ERR_BUCKET_OVERFLOW; }
    deferred = w->boxes && (w->defer_host[1] | w->defer_host[2]) != 0;
    return RB_OK;
}
static int chunk_restore(rb_world *w) {
    const char *o = static_cast<const char *>(w->opt_save.get());
    const size_t st = state_bytes(w), sn = snap_bytes(w);
    HIPCHK(hipMemcpyAsync(w->state, o, st, hipMemcpyDeviceToDevice, w->stream));
    HIPCHK(hipMemcpyAsync(w->snap[w->sp()], o + st, sn, hipMemcpyDeviceToDevice, w->stream));
    if (w->boxes) HIPCHK(hipMemcpyAsync(w->qsnap[w->sp()], o + st + sn, sn, hipMemcpyDeviceToDevice, w->stream));
    w->err_pub = false;
    HIPCHK(hipMemcpyAsync(w->err, o + st + 2 * sn, sizeof(int32_t), hipMemcpyDeviceToDevice, w->stream));
    if (w->boxes) HIPCHK(hipMemsetAsync(w->defer_cnt, 0, sizeof(int32_t) * 2, w->stream));
    w->primed = false;
    w->tile_valid_sp = -1;
    return RB_OK;
}
// twice the buckets (both tables, emptied), if under the world's limit; the
// linear layout's period gets the extra bit (refit_from_device re-splits it)
static int grow_table(rb_world *w, bool &grown) {
    grown = false;
    if (w->H * 2 > w->hmax) return RB_OK;
    HIPCHK(hipStreamSynchronize(w->stream));
    drop_graphs(w);                                   // H and the grid are captured kernel arguments
    const int64_t H = w->H * 2;
    for (int k = 0; k < 2; ++k) {
        WCHK(w->ids[k].alloc(line_bytes(H)));
        WCHK(wfill(w, w->ids[k], 0, line_bytes(H)));
        if (w->pos[k]) WCHK(w->pos[k].alloc(rb::slot_snapshot_bytes(w->esz, H)));
    }
    w->H = H;
    if (layout_linear(w->group)) w->group = period_bump(w->group);
    w->fit_valid = false;
    w->primed = false;
    w->table_grows += 1;
    grown = true;
    return RB_OK;
}

// max_partners raised to 32 (the second kernel instantiation), contact
// records resized to match
static int grow_partners(rb_world *w) {
    HIPCHK(hipStreamSynchronize(w->stream));
    drop_graphs(w);                                   // the instantiation is chosen at capture
    w->maxp = 32;
    w->maxrec = maxrec(w->n_planes, w->boxes, w->maxp);
    if (w->rec_count) {
        const size_t slots = record_slots(w);
        // (all three released before the first is allocated again)
        w->rec_partner.reset(); w->rec_kind.reset(); w->rec_dist.reset();
        WCHK(w->rec_partner.alloc(sizeof(int32_t) * slots));
        WCHK(w->rec_kind.alloc(sizeof(int32_t) * slots));
        WCHK(w->rec_dist.alloc((size_t)w->esz * slots));
    }
    w->partner_grows += 1;
    return RB_OK;
}

// the current snapshot's first N rows (x, y, z, bound radius) on the host, as doubles
int snapshot_to_host(rb_world *w, std::vector<double> &rows) {
    rows.resize((size_t)4 * w->N);
    return by_real(w->dtype, [&](auto t) -> int {
        using T = decltype(t);
        std::vector<T> sn(rows.size());
        HIPCHK(hipMemcpyAsync(sn.data(), w->snap[w->sp()], sizeof(T) * sn.size(), hipMemcpyDeviceToHost, w->stream));
        HIPCHK(hipStreamSynchronize(w->stream));
        std::copy(sn.begin(), sn.end(), rows.begin());
        return RB_OK;
    });
}

// the layout period refitted to the current positions (the snapshot, read
// back once: waits for the stream); force: fit_period's
int refit_from_device(rb_world *w, bool force) {
    std::vector<double> sn, q((size_t)7 * w->N, 0.0);
    WCHK(snapshot_to_host(w, sn));
    for (int64_t b = 0; b < w->N; ++b)
        for (int d = 0; d < 3; ++d) q[(size_t)(7 * b + d)] = sn[(size_t)(4 * b + d)];
    fit_period(w, q.data(), force);
    return RB_OK;
}

// A guarded chunk of K steps from the world's step counter (`replay(K, opt)`
// enqueues them; opt: without the box kernel): saved, run, checked, and while
// the check fails rolled back, mended and run again — K may come back
// shorter.  left: the steps of the call still to run, this chunk included.
int guarded_chunk(rb_world *w, int64_t &K, int64_t left, bool opt, double dt, double e, double mu,
                  const std::function<int(int64_t, bool)> &replay) {
    bool refitted = false;
    for (;;) {
        if (int rc = chunk_save(w)) return rc;
        w->box_kernel_on = !opt;
        const int rc = replay(K, opt);
        w->box_kernel_on = true;
        if (rc) return rc;
        int32_t err = 0;
        bool deferred = false;
        if (int rc2 = chunk_check(w, err, deferred)) return rc2;
        if (opt) w->box_stats[0] += 1;
        // bucket overflow right after a fit of one step: a real overflow
        // (reported by the caller's error check)
        const bool overflow = (err & ERR_BUCKET_OVERFLOW) && !(refitted && K == 1);
        // more sphere partners than max_partners 16: the 32-partner kernels
        const bool partners = (err & ERR_PARTNER_OVERFLOW) && w->maxp < 32;
        deferred = deferred && opt;
        if (!overflow && !deferred && !partners) {
            if (opt && w->box_backoff > 0) w->box_backoff /= 2;
            break;
        }
        if (int rc3 = chunk_restore(w)) return rc3;
        if (deferred) {
            // a box-involved pair came into range: the chunk again, from
            // its start, with the box kernel; the next chunks keep it
            w->box_stats[1] += 1;
            w->box_backoff = w->box_backoff ? std::min(2 * w->box_backoff, 64) : 1;
            w->box_skip = w->box_backoff;
            opt = false;
        }
        if (partners)
            if (int rc3 = grow_partners(w)) return rc3;
        if (overflow) {
            // the scene outgrew the layout it was fitted for: refit to
            // the chunk-start positions; if the chunk overflows again,
            // a table twice the size (one more period bit), and once the
            // table is at its limit, shorter chunks
            if (refitted) {
                bool grown = false;
                if (int rc3 = grow_table(w, grown)) return rc3;
                if (!grown) K = K > 1 ? K / 2 : 1;
            }
            if (int rc3 = refit_from_device(w)) return rc3;
            w->refits += 1;
            refitted = true;
        }
        // table headers only rise (atomicMax on generation): the
        // replay's generations must lie above every one the rolled-
        // back chunk used
        w->gen_off += (uint32_t)K + 1u;
        if (int rc3 = gen_guard(w, left + K)) return rc3;
        if (int rc3 = prime(w, dt, e, mu)) return rc3;
    }
    return RB_OK;
}

}  // namespace rb::host
