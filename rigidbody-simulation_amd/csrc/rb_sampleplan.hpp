// rb_sampleplan.hpp — how a sampled batch run (rb_batch_run_sampled) is cut
// into launches.  HIP-free: plain host C++ (tests/host_sampleplan.cpp).
//
// A run of nsteps steps records a sample after every every-th step, S =
// nsteps / every of them.  A launch runs at most `chunk` steps
// (RB_BATCH_CHUNK) and may add no more samples than the sample buffer still
// has room for; a buffer that is full, or holds samples when the run ends, is
// drained (transposed and downloaded) after the launch.  The sampling period
// runs on across launches: every launch is told how many steps lie between
// its start and its first sample (its phase).
#pragma once
#include <stdint.h>

namespace rb {

struct SampleLaunch {
    int64_t steps;      // steps of this launch, in [1, chunk]
    int64_t phase;      // the launch's step number `phase` (1-based) is its first sample; in [1, every]
    int64_t first;      // the run's samples held by the buffer before the launch (its slot offset)
    int64_t samples;    // samples this launch records: steps phase, phase + every, ... <= steps
    int64_t drain;      // samples to drain after the launch (0: none); they are the run's
    int64_t drain_at;   // samples [drain_at, drain_at + drain)
};

struct SamplePlan {
    int64_t nsteps, every, chunk;
    int64_t fit;        // samples the buffer holds (>= 1)
    int64_t done = 0;   // steps planned so far
    int64_t held = 0;   // samples in the buffer
    int64_t out = 0;    // samples drained so far

    SamplePlan(int64_t nsteps_, int64_t every_, int64_t chunk_, int64_t fit_)
        : nsteps(nsteps_), every(every_), chunk(chunk_), fit(fit_) {}

    int64_t total_samples() const { return nsteps / every; }

    // the next launch; false when the run is complete
    bool next(SampleLaunch &l) {
        if (done >= nsteps) return false;
        l.phase = every - done % every;
        l.steps = nsteps - done < chunk ? nsteps - done : chunk;
        l.samples = l.steps >= l.phase ? 1 + (l.steps - l.phase) / every : 0;
        const int64_t room = fit - held;           // >= 1: a full buffer was drained
        if (l.samples > room) {
            // end the launch at the sample that fills the buffer
            l.samples = room;
            l.steps = l.phase + (room - 1) * every;
        }
        l.first = held;
        done += l.steps;
        held += l.samples;
        l.drain = 0;
        l.drain_at = out;
        if (held > 0 && (held == fit || done == nsteps)) {
            l.drain = held;
            out += held;
            held = 0;
        }
        return true;
    }
};

}  // namespace rb
