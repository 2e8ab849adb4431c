// rb_api_shard.hip — sharded worlds: the RCCL loader, the peer-to-peer and
// halo exchanges, and the rb_shard_* / rb_p2p_* entries.
#include <dlfcn.h>

#include "rb_host.hpp"

namespace rb::host {
namespace {

// RCCL, loaded at first use: only the in-library exchange of sharded worlds
// needs it (and in a torch process the already-loaded copy is reused)
struct Rccl {
    bool tried = false, ok = false;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl &rccl() {
    static Rccl r;
    if (r.tried) return r;
    r.tried = true;
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return r;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(h, "ncclCommInitRank");
    r.AllGather = (decltype(r.AllGather))dlsym(h, "ncclAllGather");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
    r.ok = r.GetUniqueId && r.CommInitRank && r.AllGather && r.CommDestroy && r.GetErrorString;
    return r;
}

// the peer-to-peer exchange of the next snapshot and table (parity nsp)
template <typename T> P2PParams<T> make_p2p(rb_world *w, int64_t c, int nsp) {
    w->err_pub = false;
    P2PParams<T> pp{};
    pp.ins = make_insert<T>(w, nsp, 0, w->N, w->lo, w->lo + w->n_local);
    pp.dst = dp<Snap<T>>(w->snap[nsp], 0);
    pp.peer_snap = reinterpret_cast<const Snap<T> *const *>(w->peer_snap_dev + (size_t)nsp * w->P);
    pp.peer_flags = w->peer_flags_dev;
    pp.flags = w->flags;
    pp.epoch = w->epoch;
    pp.rank = (int32_t)w->rank;
    pp.P = (int32_t)w->P;
    pp.S = w->S;
    pp.timeout_ticks = 500000000;      // 5 s at 100 MHz
    pp.bounds = w->bounds + (c % 2) * BOUND_COPIES * BOUND_STRIDE;
    pp.bounds_reset = w->bounds + ((c + 1) % 2) * BOUND_COPIES * BOUND_STRIDE;
    if (w->boxes) {
        pp.peer_quat = reinterpret_cast<const T *const *>(w->peer_quat_dev + (size_t)nsp * w->P);
        pp.qdst = dp<T>(w->qsnap[nsp], 0);
    }
    return pp;
}

// the halo exchange after the step kernel of step c (next snapshot and table nsp)
template <typename T> HaloParams<T> make_halo(rb_world *w, int64_t c, int nsp) {
    w->err_pub = false;
    HaloParams<T> hp{};
    hp.ins = make_insert<T>(w, nsp, 0, 0, 0, 0);
    hp.dst = dp<Snap<T>>(w->snap[nsp], 0);
    hp.bounds = w->bounds + (c % 2) * BOUND_COPIES * BOUND_STRIDE;
    hp.bounds_reset = w->bounds + ((c + 1) % 2) * BOUND_COPIES * BOUND_STRIDE;
    hp.push_cnt = w->push_cnt;
    hp.halo_e = w->halo_e;
    hp.own = dp<Snap<T>>(w->snap[c % 2], 0);
    hp.peer_mail = reinterpret_cast<char *const *>(w->peer_flags_dev.get());
    hp.mail = reinterpret_cast<const char *>(w->flags.get());
    hp.lay = MailLayout::make(w->P, w->S, w->esz, w->boxes);
    hp.epoch = w->epoch;
    hp.rank = (int32_t)w->rank;
    hp.P = (int32_t)w->P;
    hp.n_local = w->n_local;
    hp.lo = w->lo;
    hp.S = w->S;
    hp.timeout_ticks = 500000000;      // 5 s at 100 MHz
    hp.quat = w->boxes ? dp<T>(w->qsnap[nsp], 0) : nullptr;
    return hp;
}

// in-place all-gather of the snapshot of parity sp (and, box worlds, of the
// orientation snapshot: [P][S][4] the same way)
int rccl_gather(rb_world *w, int sp, hipStream_t s) {
    const size_t n = (size_t)4 * w->S;
    const ncclDataType_t ty = w->dtype == RB_F64 ? ncclFloat64 : ncclFloat32;
    for (int k = 0; k < (w->boxes ? 2 : 1); ++k) {
        char *buf = static_cast<char *>(k == 0 ? w->snap[sp].get() : w->qsnap[sp].get());
        const ncclResult_t r = rccl().AllGather(buf + (size_t)w->esz * n * w->rank, buf, n, ty, w->comm, s);
        if (r != ncclSuccess) return fail(RB_ENODEV, "ncclAllGather: %s", rccl().GetErrorString(r));
    }
    return RB_OK;
}

// the insert of every other rank's bodies into the table of parity nsp,
// reading the freshly exchanged snapshot (own ones went in from the step kernel)
hipError_t insert_others(rb_world *w, int nsp, hipStream_t s) {
    return by_real(w->dtype, [&](auto t) {
        using T = decltype(t);
        return launch_insert<T>(make_insert<T>(w, nsp, 0, w->N, w->lo, w->lo + w->n_local), s);
    });
}

// IPC handles per rank: both snapshots, the mailbox, (box worlds) both
// orientation snapshots
int p2p_nhandles(const rb_world *w) { return w->boxes ? 5 : 3; }

// both parities of the own cell bounds empty: the next step kernel folds
// into one, the exchange after it resets the other
int reset_bounds(rb_world *w) {
    if (!w->bounds) WCHK(w->bounds.alloc(sizeof(int32_t) * 2 * BOUND_COPIES * BOUND_STRIDE));
    std::vector<int32_t> b((size_t)2 * BOUND_COPIES * BOUND_STRIDE, 0);
    for (int k = 0; k < 2 * BOUND_COPIES; ++k)
        for (int d = 0; d < 3; ++d) { b[(size_t)k * BOUND_STRIDE + d] = INT32_MAX; b[(size_t)k * BOUND_STRIDE + 3 + d] = INT32_MIN; }
    WCHK(wput(w, w->bounds, b.data(), sizeof(int32_t) * b.size()));
    return RB_OK;
}

}  // namespace

// The in-library exchange after the step kernel of step c (which put the own
// bodies' new positions in this rank's slice of the next snapshot): the
// in-place all-gather of that snapshot, then the insert of every other
// rank's bodies into the next table (as rb_shard_exchange_done).
int shard_exchange(rb_world *w, hipStream_t s, int64_t c) {
    const int nsp = 1 - (int)(c % 2);
    if (w->p2p) {
        const hipError_t pe = by_real(w->dtype, [&](auto t) {
            using T = decltype(t);
            return w->halo ? launch_halo_exchange<T>(make_halo<T>(w, c, nsp), s)
                           : launch_p2p_exchange<T>(make_p2p<T>(w, c, nsp), s);
        });
        HIPCHK(pe);
        return RB_OK;
    }
    if (int rc = rccl_gather(w, nsp, s)) return rc;
    HIPCHK(insert_others(w, nsp, s));
    return RB_OK;
}
// one sharded step: step kernel, then the exchange
int shard_one(rb_world *w, hipStream_t s, int64_t c, double dt, double e, double mu, double thr) {
    const int rc = launch_one(w, s, c, dt, e, mu, thr);
    return rc ? rc : shard_exchange(w, s, c);
}

// the halo pushes of a run's first step test against the bounds of the
// current positions (the insert kernels publish them after)
int halo_prime(rb_world *w) {
    const hipError_t he = by_real(w->dtype, [&](auto t) {
        using T = decltype(t);
        return launch_halo_prime<T>(make_halo<T>(w, w->c, w->sp()), w->stream);
    });
    HIPCHK(he);
    return RB_OK;
}

// a world's communicator and peer mappings (free_world; the exchange buffers go with the world)
void shard_release(rb_world *w) {
    if (w->comm) (void)rccl().CommDestroy(w->comm);
    for (void *q : w->ipc_opened) (void)hipIpcCloseMemHandle(q);
}

}  // namespace rb::host

using namespace rb::host;

extern "C" {

int rb_shard_step(rb_world *w, double dt, double e, double mu, double thr) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w) return fail(RB_EINVAL, "null world");
    if (w->law != RB_LAW_MUJOCO) return fail(RB_EUNSUPPORTED, "sharded stepping supports the default contact law only");
    if (!(dt > 0) || !(e >= 0) || !(mu >= 0) || !(thr >= 0)) return fail(RB_EINVAL, "invalid step parameters");
    HIPCHK(hipSetDevice(w->device));
    if (int rc = gen_guard(w, 1)) return rc;
    if (!w->primed) { int rc = prime(w); if (rc) return rc; }
    w->state_version += 1;
    if (w->timing) return timed_launch(w, dt, e, mu, thr);
    return launch_one(w, w->stream, w->c, dt, e, mu, thr);
}

int rb_shard_exchange_done(rb_world *w) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w) return fail(RB_EINVAL, "null world");
    HIPCHK(hipSetDevice(w->device));
    HIPCHK(insert_others(w, 1 - w->sp(), w->stream));
    ++w->c;
    return RB_OK;
}

int rb_gpos_buffer(rb_world *w, void **dev_ptr, int64_t *shard_elems, int32_t *elem_bytes) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w) return fail(RB_EINVAL, "null world");
    if (dev_ptr) *dev_ptr = w->snap[1 - w->sp()];
    if (shard_elems) *shard_elems = 4 * w->S;
    if (elem_bytes) *elem_bytes = w->esz;
    return RB_OK;
}

int rb_gquat_buffer(rb_world *w, void **dev_ptr, int64_t *shard_elems, int32_t *elem_bytes) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w) return fail(RB_EINVAL, "null world");
    if (dev_ptr) *dev_ptr = w->boxes ? w->qsnap[1 - w->sp()] : nullptr;
    if (shard_elems) *shard_elems = w->boxes ? 4 * w->S : 0;
    if (elem_bytes) *elem_bytes = w->esz;
    return RB_OK;
}

int rb_comm_unique_id(void *id, int32_t bytes) {
    ApiScope api_scope_(-1);
    if (!id || bytes < (int32_t)sizeof(ncclUniqueId)) return fail(RB_EINVAL, "id buffer must hold %d bytes", (int)sizeof(ncclUniqueId));
    if (!rccl().ok) return fail(RB_ENODEV, "RCCL (librccl.so) not available");
    ncclUniqueId u;
    const ncclResult_t r = rccl().GetUniqueId(&u);
    if (r != ncclSuccess) return fail(RB_ENODEV, "ncclGetUniqueId: %s", rccl().GetErrorString(r));
    memcpy(id, &u, sizeof(u));
    return RB_OK;
}

int rb_shard_comm_init(rb_world *w, const void *id, int32_t bytes) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w || !id || bytes < (int32_t)sizeof(ncclUniqueId)) return fail(RB_EINVAL, "null world or short id");
    if (w->comm) return fail(RB_EINVAL, "communicator already initialised");
    if (!rccl().ok) return fail(RB_ENODEV, "RCCL (librccl.so) not available");
    HIPCHK(hipSetDevice(w->device));
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclResult_t r = rccl().CommInitRank(&w->comm, (int)w->P, u, (int)w->rank);
    if (r != ncclSuccess) { w->comm = nullptr; return fail(RB_ENODEV, "ncclCommInitRank: %s", rccl().GetErrorString(r)); }
    // first collective outside any graph capture (connection setup); the
    // snapshots are replicated, so the in-place gather leaves them unchanged
    if (int rc = rccl_gather(w, w->sp(), w->stream)) return rc;
    HIPCHK(hipStreamSynchronize(w->stream));
    drop_graphs(w);
    return RB_OK;
}

int rb_p2p_handles(rb_world *w, void *out, int64_t cap, int64_t *len) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w || !len) return fail(RB_EINVAL, "null argument");
    const int nh = p2p_nhandles(w);
    const int64_t need = nh * (int64_t)sizeof(hipIpcMemHandle_t);
    *len = need;
    if (!out) return RB_OK;
    if (cap < need) return fail(RB_EINVAL, "handle buffer needs %lld bytes", (long long)need);
    HIPCHK(hipSetDevice(w->device));
    if (!w->flags) {
        // the mailbox, uncached: peers write it over xGMI while this rank's
        // kernels poll and read it
        const MailLayout lay = MailLayout::make(w->P, w->S, w->esz, w->boxes);
        WCHK(w->flags.alloc_uncached((size_t)lay.bytes));
        WCHK(wfill(w, w->flags, 0, (size_t)lay.bytes));
        HIPCHK(hipStreamSynchronize(w->stream));     // (the peers map it next)
    }
    hipIpcMemHandle_t h[5];
    HIPCHK(hipIpcGetMemHandle(&h[0], w->snap[0]));
    HIPCHK(hipIpcGetMemHandle(&h[1], w->snap[1]));
    HIPCHK(hipIpcGetMemHandle(&h[2], w->flags));
    if (w->boxes) {
        HIPCHK(hipIpcGetMemHandle(&h[3], w->qsnap[0]));
        HIPCHK(hipIpcGetMemHandle(&h[4], w->qsnap[1]));
    }
    memcpy(out, h, need);
    return RB_OK;
}

int rb_p2p_connect(rb_world *w, const void *all, int64_t len) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w || !all) return fail(RB_EINVAL, "null argument");
    const int nh = p2p_nhandles(w);
    const int64_t blob = nh * (int64_t)sizeof(hipIpcMemHandle_t);
    if (len != blob * w->P) return fail(RB_EINVAL, "expected %lld bytes of handles (P blobs)", (long long)(blob * w->P));
    if (!w->flags) return fail(RB_EINVAL, "rb_p2p_handles first");
    if (w->p2p) return fail(RB_EINVAL, "already connected");
    HIPCHK(hipSetDevice(w->device));
    std::vector<void *> snaps(2 * (size_t)w->P, nullptr), quats(2 * (size_t)w->P, nullptr);
    std::vector<int64_t *> flags((size_t)w->P, nullptr);
    const char *b = static_cast<const char *>(all);
    for (int64_t q = 0; q < w->P; ++q) {
        if (q == w->rank) {
            snaps[(size_t)q] = w->snap[0];
            snaps[(size_t)(w->P + q)] = w->snap[1];
            flags[(size_t)q] = w->flags;
            quats[(size_t)q] = w->qsnap[0];
            quats[(size_t)(w->P + q)] = w->qsnap[1];
            continue;
        }
        hipIpcMemHandle_t h[5];
        memcpy(h, b + blob * q, (size_t)blob);
        void *ptr[5] = {};
        for (int k = 0; k < nh; ++k) {
            if (hipIpcOpenMemHandle(&ptr[k], h[k], hipIpcMemLazyEnablePeerAccess) != hipSuccess)
                return fail(RB_ENODEV, "hipIpcOpenMemHandle(rank %lld, buffer %d) failed", (long long)q, k);
            w->ipc_opened.push_back(ptr[k]);
        }
        snaps[(size_t)q] = ptr[0];
        snaps[(size_t)(w->P + q)] = ptr[1];
        flags[(size_t)q] = static_cast<int64_t *>(ptr[2]);
        quats[(size_t)q] = ptr[3];
        quats[(size_t)(w->P + q)] = ptr[4];
    }
    if (w->boxes) {
        WCHK(w->peer_quat_dev.alloc(sizeof(void *) * quats.size()));
        WCHK(wput(w, w->peer_quat_dev, quats.data(), sizeof(void *) * quats.size()));
    }
    WCHK(w->peer_snap_dev.alloc(sizeof(void *) * snaps.size()));
    WCHK(w->peer_flags_dev.alloc(sizeof(int64_t *) * flags.size()));
    WCHK(w->epoch.alloc(sizeof(int64_t)));
    WCHK(wput(w, w->peer_snap_dev, snaps.data(), sizeof(void *) * snaps.size()));
    WCHK(wput(w, w->peer_flags_dev, flags.data(), sizeof(int64_t *) * flags.size()));
    WCHK(wfill(w, w->epoch, 0, sizeof(int64_t)));
    WCHK(wfill(w, w->flags, 0, sizeof(int64_t) * w->P));
    // the own cell bounds (both modes filter the peers' bodies by them)
    if (int rc = reset_bounds(w)) return rc;
    HIPCHK(hipStreamSynchronize(w->stream));         // (the flags zeroed before any peer's step can flag)
    w->p2p = true;
    drop_graphs(w);
    return RB_OK;
}

int rb_p2p_halo(rb_world *w, int32_t enable) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w) return fail(RB_EINVAL, "null world");
    if (!w->p2p) return fail(RB_EINVAL, "rb_p2p_halo before rb_p2p_connect");
    HIPCHK(hipSetDevice(w->device));
    HIPCHK(hipStreamSynchronize(w->stream));
    if (enable) {
        if (!w->push_cnt) WCHK(w->push_cnt.alloc(sizeof(int32_t) * w->P));
        if (!w->halo_e) WCHK(w->halo_e.alloc(sizeof(int64_t)));
        if (int rc = reset_bounds(w)) return rc;
        WCHK(wfill(w, w->push_cnt, 0, sizeof(int32_t) * w->P));
    }
    if (w->halo != (enable != 0)) drop_graphs(w);
    w->halo = enable != 0;
    return RB_OK;
}

int rb_shard_run(rb_world *w, int64_t nsteps, double dt, double e, double mu, double thr) {
    ApiScope api_scope_(w ? w->device : -1);
    if (!w) return fail(RB_EINVAL, "null world");
    return enqueue_steps(w, nsteps, dt, e, mu, thr, true);
}

}  // extern "C"
