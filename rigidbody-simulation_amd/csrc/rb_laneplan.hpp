// rb_laneplan.hpp — how the bodies of a one-wave batch with a population
// (rb_batch_set_population) are mapped to lanes.  HIP-free: plain host C++
// (tests/host_laneplan.cpp).
//
// Environment e holds n[e] present bodies (1..M, M <= 64), rows e * M + b for
// b < n[e].  Whole environments are packed into waves of 64 lanes in
// environment order, next-fit: an environment that does not fit the rest of a
// wave starts the next one.  So a wave covers a contiguous range of
// environments, an environment's lanes are consecutive in one wave in body
// order, and with every count equal to M a wave holds floor(64 / M)
// environments, the fixed mapping of the batch kernels (rb_batch.hip).
// Absent bodies have no lane; the lanes left over in a wave are idle (row -1).
#pragma once
#include <stdint.h>
#include <vector>

namespace rb {

constexpr int LANEPLAN_WAVE = 64;

struct LanePlan {
    std::vector<int32_t> wave_env0;   // [waves + 1] a wave's first environment; wave_env0[waves] = E
    std::vector<int32_t> lane_row;    // [waves * 64] the lane's row e * M + b, or -1: idle
    int32_t waves = 0;
    int32_t epw_max = 0;              // most environments of one wave
};

// n: E counts, each in [1, M]; M in [1, 64]; E * M < 2^31.  false (and an
// empty plan) for arguments outside that.
inline bool lane_plan(const int32_t *n, int64_t E, int32_t M, LanePlan &out) {
    out = LanePlan{};
    if (!n || E < 1 || M < 1 || M > LANEPLAN_WAVE || E > (int64_t)INT32_MAX / M) return false;
    for (int64_t e = 0; e < E; ++e)
        if (n[e] < 1 || n[e] > M) return false;
    int32_t used = LANEPLAN_WAVE;     // lanes taken in the open wave (full: the first environment opens one)
    for (int64_t e = 0; e < E; ++e) {
        if (used + n[e] > LANEPLAN_WAVE) {
            out.wave_env0.push_back((int32_t)e);
            out.lane_row.resize(out.lane_row.size() + LANEPLAN_WAVE, -1);
            ++out.waves;
            used = 0;
        }
        const size_t at = (size_t)(out.waves - 1) * LANEPLAN_WAVE + (size_t)used;
        for (int32_t b = 0; b < n[e]; ++b) out.lane_row[at + (size_t)b] = (int32_t)(e * M + b);
        used += n[e];
        const int32_t here = (int32_t)e - out.wave_env0.back() + 1;
        if (here > out.epw_max) out.epw_max = here;
    }
    out.wave_env0.push_back((int32_t)E);
    return true;
}

}  // namespace rb
