// rb_api_world_dev.hip — the device-resident boundary of a world:
// rb_get_state_dev / rb_set_state_dev / rb_set_xfrc_dev.  The caller's arrays
// are device memory; every call is enqueued on the world's stream and, but
// for the cases the header names, does not wait (kernels: rb_world_dev.hip).
#include "rb_host.hpp"
#include "rb_world_dev.hpp"

namespace rb::host {

// what all three entries refuse, before any device call
static int dev_refuse(const rb_world *w, bool have_array, int32_t io_dtype) {
    if (!w) return fail(RB_EINVAL, "null world");
    if (!have_array) return fail(RB_EINVAL, "null argument");
    if (io_dtype != RB_F64 && io_dtype != RB_F32) return fail(RB_EINVAL, "io_dtype %d is neither RB_F64 nor RB_F32", io_dtype);
    if (w->P > 1)
        return fail(RB_EUNSUPPORTED, "the device-resident boundary is for world_size 1 (a shard's boundary is rb_gpos_buffer)");
    return RB_OK;
}

template <typename T> static WDevState<T> make_wdev(rb_world *w) {
    WDevState<T> p{};
    p.snap = dp<Snap<T>>(w->snap[w->sp()], 0);
    p.quat = w->boxes ? dp<T>(w->qsnap[w->sp()], 0) : nullptr;
    p.st = BodyState<T>{dp<T>(w->state, 0), w->S};
    p.bound = dp<T>(w->consts, 7 * w->Npad);
    p.N = w->N;
    p.balls = w->law == RB_LAW_BALLS;
    return p;
}

// f(T{}, IO{}): T the world's real type, IO the caller's element type
template <typename F> static auto by_real_io(const rb_world *w, int32_t io_dtype, F &&f) {
    return by_real(w->dtype, [&](auto t) { return by_real(io_dtype, [&](auto io) { return f(t, io); }); });
}

}  // namespace rb::host

using namespace rb::host;

extern "C" {

int rb_get_state_dev(rb_world *w, void *qpos, void *qvel, int32_t io_dtype) {
    ApiScope api_scope_(w ? w->device : -1);
    if (int rc = dev_refuse(w, qpos || qvel, io_dtype)) return rc;
    HIPCHK(hipSetDevice(w->device));
    if (int rc = finish_pending(w)) return rc;
    HIPCHK(by_real_io(w, io_dtype, [&](auto t, auto io) {
        using T = decltype(t);
        using IO = decltype(io);
        return launch_wdev_state_out<T, IO>(make_wdev<T>(w), (IO *)qpos, (IO *)qvel, w->stream);
    }));
    return RB_OK;
}

int rb_set_state_dev(rb_world *w, const void *qpos, const void *qvel, int32_t io_dtype, int32_t refit) {
    ApiScope api_scope_(w ? w->device : -1);
    if (int rc = dev_refuse(w, qpos && qvel, io_dtype)) return rc;
    HIPCHK(hipSetDevice(w->device));
    if (int rc = finish_pending(w)) return rc;
    HIPCHK(by_real_io(w, io_dtype, [&](auto t, auto io) {
        using T = decltype(t);
        using IO = decltype(io);
        return launch_wdev_state_in<T, IO>(make_wdev<T>(w), (const IO *)qpos, (const IO *)qvel, w->stream);
    }));
    // rb_set_state's bookkeeping
    w->primed = false;
    w->tile_valid_sp = -1;
    w->tile_fit_valid = false;                           // (refitted at the next tile run)
    if (w->tile_mode_init == -1 && w->tile_mode == 0) {   // a new state: auto mode may try the form again
        w->tile_mode = -1;
        w->tile_backoff = w->tile_skip = 0;
    }
    w->state_version += 1;
    w->mirror_version = -1;                              // the pinned staging no longer equals the state
    // the layout's period fitted to the new positions, as rb_set_state fits
    // it to the host copy: here from the snapshot read back (waits)
    if (refit) WCHK(refit_from_device(w, false));
    return RB_OK;
}

int rb_set_xfrc_dev(rb_world *w, const void *xfrc, int32_t io_dtype) {
    ApiScope api_scope_(w ? w->device : -1);
    if (int rc = dev_refuse(w, xfrc != nullptr, io_dtype)) return rc;
    HIPCHK(hipSetDevice(w->device));
    if (int rc = finish_pending(w)) return rc;
    if (!w->xfrc) {
        // (graphs capture whether a step reads applied forces: rb_set_xfrc)
        HIPCHK(hipStreamSynchronize(w->stream));
        drop_graphs(w);
        WCHK(w->xfrc.alloc((size_t)w->esz * 6 * w->S));
        WCHK(wfill(w, w->xfrc, 0, (size_t)w->esz * 6 * w->S));
    }
    // steps in flight read the old forces: they precede the kernel on the stream
    HIPCHK(by_real_io(w, io_dtype, [&](auto t, auto io) {
        using T = decltype(t);
        using IO = decltype(io);
        return launch_wdev_xfrc_in<T, IO>((const IO *)xfrc, dp<T>(w->xfrc, 0), w->N, w->S, w->stream);
    }));
    return RB_OK;
}

}  // extern "C"
