// rb_api_common.hip — what every unit of the implementation of include/rbhip.h
// shares at run time: the thread gate's state, the error text, the grow-only
// device buffer and the device-memory pointer check of worlds and batches.
//
// A world owns its device buffers — struct-of-arrays state, replicated
// constants, two ping-pong position snapshots (which double as the
// replicated exchange buffer of sharded worlds) and two alternating
// broadphase tables (generation-tagged bucket lines, never cleared) — and
// enqueues all work on one HIP stream.  A step's buffers are fixed by the
// step counter's parity (and table generations live on the device), so
// multi-step calls are captured once per parity into a hipGraph (one kernel
// node per step) and replayed.  The other units are rb_api_*.hip;
// rb_host.hpp declares what crosses them.
#include <stdarg.h>

#include <condition_variable>
#include <mutex>
#include <string>

#include "rb_host.hpp"

static_assert(CK_SPHERE_BOX == RB_CK_SPHERE_BOX && CK_BOX_BOX0 == RB_CK_BOX_BOX0 && CK_BOX_EDGE == RB_CK_BOX_EDGE,
              "contact kinds");

// Threads.  A graph capture on one thread's stream is invalidated by a
// null-stream or device-wide call (hipMalloc, hipMemset, hipMemcpy, hipFree,
// ...) that another thread makes on the same device meanwhile, and that call
// fails too (seen with two threads creating, stepping and destroying their
// own worlds).  So every entry point runs inside an ApiScope of its world's
// device, and a capture (graph_replay) inside a CaptureScope: a capture on
// device d starts once no other thread is inside an entry point on d (other
// than capturing too), and no entry point on d starts while a capture on d
// runs.  Captures of several threads may overlap; a thread working on one
// device never waits for a capture on another.  Entry points with no device
// (rb_comm_unique_id) or no valid world gate every device.
namespace {
constexpr int GATE_DEVICES = 64;
struct Gate {
    std::mutex m;
    std::condition_variable cv;
    int active[GATE_DEVICES] = {};      // threads inside an entry point on device d, not capturing
    int capturing[GATE_DEVICES] = {};   // threads inside a capture on device d
    int active_all = 0;                 // threads inside a device-less entry point
    int capturing_any = 0;
};
Gate &gate() {
    static Gate g;
    return g;
}
int gate_dev(int d) { return d >= 0 && d < GATE_DEVICES ? d : -1; }
thread_local int t_api_depth = 0;
thread_local int t_api_dev = -1;

thread_local std::string g_err;
}  // namespace

namespace rb::host {

ApiScope::ApiScope(int device) {
    if (t_api_depth++ == 0) {
        const int d = gate_dev(device);
        t_api_dev = d;
        Gate &g = gate();
        std::unique_lock<std::mutex> l(g.m);
        g.cv.wait(l, [&] { return d < 0 ? g.capturing_any == 0 : g.capturing[d] == 0; });
        if (d < 0) ++g.active_all; else ++g.active[d];
    }
}
ApiScope::~ApiScope() {
    if (--t_api_depth == 0) {
        Gate &g = gate();
        std::lock_guard<std::mutex> l(g.m);
        if (t_api_dev < 0) --g.active_all; else --g.active[t_api_dev];
        g.cv.notify_all();
    }
}
CaptureScope::CaptureScope() : d(t_api_dev < 0 ? 0 : t_api_dev) {
    Gate &g = gate();
    std::unique_lock<std::mutex> l(g.m);
    if (t_api_dev < 0) --g.active_all; else --g.active[d];
    ++g.capturing[d];
    ++g.capturing_any;
    g.cv.wait(l, [&] { return g.active[d] == 0 && g.active_all == 0; });
}
CaptureScope::~CaptureScope() {
    Gate &g = gate();
    std::unique_lock<std::mutex> l(g.m);
    --g.capturing[d];
    --g.capturing_any;
    g.cv.notify_all();
    g.cv.wait(l, [&] { return g.capturing[d] == 0; });
    if (t_api_dev < 0) ++g.active_all; else ++g.active[d];
}

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int err_to_code(int32_t bits) {
    if (bits & ERR_EXCHANGE) return fail(RB_ENODEV, "device: peer-to-peer exchange timed out (a peer rank did not reach the step)");
    if (bits & ERR_HALO_MOVE)
        return fail(RB_EDOM, "device: a body moved more than one broadphase cell in one step (the halo exchange "
                             "cannot guarantee its partners; use full peer reads: rb_p2p_halo(w, 0))");
    if (bits & ERR_DOMAIN) return fail(RB_EDOM, "device: non-finite or out-of-range body position");
    if (bits & ERR_UNSUPPORTED)
        return fail(RB_EUNSUPPORTED, "device: box-involved pair within contact range with no box kernel to take it");
    if (bits & ERR_PARTNER_OVERFLOW) return fail(RB_EOVERFLOW, "device: a body has more sphere partners than max_partners");
    if (bits & ERR_BUCKET_OVERFLOW) return fail(RB_EOVERFLOW, "device: more than 30 bodies hashed to one broadphase bucket");
    return RB_OK;
}

int grow(void **buf, size_t *cap, size_t need) {
    if (need <= *cap) return RB_OK;
    if (*buf) { HIPCHK(hipFree(*buf)); *buf = nullptr; }
    *cap = 0;
    HIPCHK(hipMalloc(buf, need));
    *cap = need;
    return RB_OK;
}

void DevMem::reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
}
int DevMem::alloc_uncached(size_t n) {
    reset();
    HIPCHK(hipExtMallocWithFlags(&p, n, hipDeviceMallocUncached));
    bytes = n;
    return RB_OK;
}
void HostMem::reset() {
    if (p) (void)hipHostFree(p);
    p = d = nullptr;
}
int HostMem::alloc(size_t n, unsigned flags) {
    reset();
    HIPCHK(hipHostMalloc(&p, n, flags));
    if (flags & hipHostMallocMapped) HIPCHK(hipHostGetDevicePointer(&d, p, 0));
    return RB_OK;
}

int dev_ptrs(int device, const char *owner, std::initializer_list<std::pair<const void *, const char *>> arrays) {
    for (const auto &[p, name] : arrays) {
        if (!p) continue;
        hipPointerAttribute_t a{};
        if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeDevice) {
            (void)hipGetLastError();
            return fail(RB_EINVAL, "%s is not device memory (a host pointer?)", name);
        }
        if (a.device != device)
            return fail(RB_EINVAL, "%s is memory of device %d, the %s is on device %d", name, a.device, owner, device);
    }
    return RB_OK;
}

}  // namespace rb::host

extern "C" {

const char *rb_last_error(void) { return g_err.c_str(); }
const char *rb_version(void) { return "librbhip 0.4 (gfx950, HIP)"; }

}  // extern "C"
