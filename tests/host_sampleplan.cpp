// The launch plan of a sampled batch run (csrc/rb_sampleplan.hpp) as plain
// host C++: every sampled step exactly once and in order, no launch past the
// chunk or the buffer, the sampling phase carried across launches, every step
// run.  Exit status 0: all checks passed.
#include <stdint.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "rb_sampleplan.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            ++failures;                                           \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                         \
            fprintf(stderr, "\n");                                \
        }                                                         \
    } while (0)

// walks the plan as the host code does: a buffer of `fit` slots, filled by
// the launches and emptied by the drains into the list of sampled steps
static void check_plan(int64_t nsteps, int64_t every, int64_t chunk, int64_t fit, int64_t want_launches) {
    rb::SamplePlan plan(nsteps, every, chunk, fit);
    rb::SampleLaunch l;
    std::vector<int64_t> buffer, out;     // global step numbers (1-based) of the samples held / drained
    int64_t step = 0, launches = 0;
    while (plan.next(l)) {
        ++launches;
        CHECK(launches <= nsteps, "(%lld, %lld): the plan does not end", (long long)nsteps, (long long)every);
        if (launches > nsteps) return;
        CHECK(l.steps >= 1 && l.steps <= chunk, "launch of %lld steps", (long long)l.steps);
        CHECK(l.phase >= 1 && l.phase <= every, "phase %lld", (long long)l.phase);
        // the phase continues the period of the whole run
        CHECK((step + l.phase) % every == 0, "phase %lld at step %lld", (long long)l.phase, (long long)step);
        CHECK(l.first == (int64_t)buffer.size(), "first %lld, buffer holds %zu", (long long)l.first, buffer.size());
        // what the kernel does: count down to the next sample
        int64_t until = l.phase, stored = 0;
        for (int64_t s = 1; s <= l.steps; ++s) {
            if (--until == 0) {
                CHECK(l.first + stored < fit, "slot %lld of %lld", (long long)(l.first + stored), (long long)fit);
                buffer.push_back(step + s);
                ++stored;
                until = every;
            }
        }
        CHECK(stored == l.samples, "launch stores %lld, plan says %lld", (long long)stored, (long long)l.samples);
        step += l.steps;
        if (l.drain) {
            CHECK(l.drain == (int64_t)buffer.size(), "drain %lld of %zu", (long long)l.drain, buffer.size());
            CHECK(l.drain_at == (int64_t)out.size(), "drain_at %lld, %zu out", (long long)l.drain_at, out.size());
            out.insert(out.end(), buffer.begin(), buffer.end());
            buffer.clear();
        } else {
            CHECK((int64_t)buffer.size() < fit, "a full buffer is not drained");
        }
    }
    CHECK(step == nsteps, "%lld steps run of %lld", (long long)step, (long long)nsteps);
    CHECK(buffer.empty(), "%zu samples never drained", buffer.size());
    CHECK((int64_t)out.size() == nsteps / every && plan.total_samples() == nsteps / every, "%zu samples of %lld",
          out.size(), (long long)(nsteps / every));
    for (size_t k = 0; k < out.size(); ++k)
        CHECK(out[k] == (int64_t)(k + 1) * every, "sample %zu is step %lld", k, (long long)out[k]);
    if (want_launches >= 0)
        CHECK(launches == want_launches, "(%lld, %lld, fit %lld): %lld launches, expected %lld", (long long)nsteps,
              (long long)every, (long long)fit, (long long)launches, (long long)want_launches);
}

int main() {
    const int64_t INF = std::numeric_limits<int64_t>::max();
    check_plan(600, 7, 256, INF, 3);      // 256 + 256 + 88; step 259 is local step 3 of the second launch
    check_plan(600, 7, 256, 3, -1);       // 21 steps per launch
    check_plan(256, 256, 256, 1, 1);      // the sample at the launch's last step
    check_plan(255, 256, 256, 1, 1);      // no sample at all
    check_plan(0, 1, 256, 1, 0);
    check_plan(1000, 1, 256, 5, 200);     // 5 steps per launch
    check_plan(513, 512, 256, 1, 3);      // 256 + 256 (sample at its end) + 1
    // the second launch of (600, 7): phase 3
    {
        rb::SamplePlan plan(600, 7, 256, INF);
        rb::SampleLaunch l;
        plan.next(l);
        CHECK(l.steps == 256 && l.phase == 7 && l.samples == 36 && l.drain == 0, "first launch");
        plan.next(l);
        CHECK(l.steps == 256 && l.phase == 3 && l.first == 36 && l.samples == 37 && l.drain == 0, "second launch");
        plan.next(l);
        CHECK(l.steps == 88 && l.phase == 6 && l.first == 73 && l.samples == 12 && l.drain == 85 && l.drain_at == 0,
              "third launch");
        CHECK(!plan.next(l), "a fourth launch");
    }
    // a sweep of small cases
    for (int64_t n = 0; n <= 40; ++n)
        for (int64_t every = 1; every <= 12; ++every)
            for (int64_t chunk = 1; chunk <= 9; chunk += 4)
                for (int64_t fit = 1; fit <= 4; ++fit) check_plan(n, every, chunk, fit, -1);
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("host_sampleplan: ok\n");
    return 0;
}
