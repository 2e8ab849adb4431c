// rb_hostpool.hpp — the host thread pool of rb_set_state / rb_get_state
// (rb_api_state.hip).  Standard library only: compiles without HIP
// (tests/host_units.cpp).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace rb {
namespace host __attribute__((visibility("hidden"))) {

// A few host threads for the boundary's copies and compares: rb_set_state
// and rb_get_state move 13 doubles per body (6.8 MB at 65,536 bodies), which
// one core copies in ~0.6 ms.  Workers wait on a condition variable; a job
// is cut into pieces taken from an atomic counter by the workers and the
// caller.  Small jobs run inline.
class HostPool {
    std::vector<std::thread> th_;
    std::mutex m_, job_m_;
    std::condition_variable cv_, done_cv_;
    uint64_t gen_ = 0;
    int busy_ = 0;
    bool stop_ = false;
    const std::function<void(size_t, size_t)> *fn_ = nullptr;
    size_t n_ = 0, pieces_ = 0;
    std::atomic<size_t> next_{0}, done_{0};
    void work() {
        for (size_t k; (k = next_.fetch_add(1)) < pieces_;) {
            (*fn_)(n_ * k / pieces_, n_ * (k + 1) / pieces_);
            done_.fetch_add(1);
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(m_);
            cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
            if (stop_) return;
            seen = gen_;
            ++busy_;
            lk.unlock();
            work();
            lk.lock();
            --busy_;
            lk.unlock();
            done_cv_.notify_all();
        }
    }

  public:
    HostPool() {
        int want = 8;
        if (const char *ev = getenv("OMP_NUM_THREADS")) want = atoi(ev);
        if (const char *ev = getenv("RBHIP_HOST_THREADS")) want = atoi(ev);
        want = std::max(1, std::min(want, 16));
        for (int k = 1; k < want; ++k) th_.emplace_back([this] { loop(); });
    }
    ~HostPool() {
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    static HostPool &get() { static HostPool p; return p; }
    // fn(lo, hi) over [0, n)
    void run(size_t n, const std::function<void(size_t, size_t)> &fn) {
        if (th_.empty() || n < (size_t(1) << 15)) { fn(0, n); return; }
        std::lock_guard<std::mutex> jl(job_m_);
        {
            std::unique_lock<std::mutex> lk(m_);
            done_cv_.wait(lk, [&] { return busy_ == 0; });     // (no worker still in the last job)
            fn_ = &fn; n_ = n; pieces_ = 4 * (th_.size() + 1);
            next_ = 0; done_ = 0;
            ++gen_;
        }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> lk(m_);
        done_cv_.wait(lk, [&] { return done_.load() == pieces_ && busy_ == 0; });
    }
};
// fn(array, lo, hi) over [0, n0) of array 0 and [0, n1) of array 1, in one
// pool run (one wake-up of the workers for both of a state's arrays)
template <typename F> void par_two(size_t n0, size_t n1, const F &fn) {
    HostPool::get().run(n0 + n1, [&](size_t lo, size_t hi) {
        if (lo < n0) fn(0, lo, std::min(hi, n0));
        if (hi > n0) fn(1, std::max(lo, n0) - n0, hi - n0);
    });
}
// dst_k[0, n_k) = src_k[0, n_k), k = 0, 1
inline void par_copy2(double *d0, const double *s0, size_t n0, double *d1, const double *s1, size_t n1) {
    par_two(n0, n1, [&](int k, size_t lo, size_t hi) {
        if (k == 0) memcpy(d0 + lo, s0 + lo, sizeof(double) * (hi - lo));
        else memcpy(d1 + lo, s1 + lo, sizeof(double) * (hi - lo));
    });
}
inline bool par_equal2(const double *a0, const double *b0, size_t n0, const double *a1, const double *b1, size_t n1) {
    std::atomic<int> diff{0};
    par_two(n0, n1, [&](int k, size_t lo, size_t hi) {
        const double *a = k ? a1 : a0, *b = k ? b1 : b0;
        if (!diff.load(std::memory_order_relaxed) && memcmp(a + lo, b + lo, sizeof(double) * (hi - lo)) != 0) diff = 1;
    });
    return diff.load() == 0;
}

}  // namespace host
}  // namespace rb
