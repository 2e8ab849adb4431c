// The lane plan of a batch with a population (csrc/rb_laneplan.hpp) as plain
// host C++: every present body exactly one lane, an environment's lanes
// consecutive in one wave in body order, environments in order across waves,
// idle lanes -1, uniform counts reproducing floor(64 / M) environments per
// wave.  Exit status 0: all checks passed.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "rb_laneplan.hpp"

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

// the properties every plan has; want_waves < 0: not checked
static rb::LanePlan check_plan(const std::vector<int32_t> &n, int32_t M, int want_waves) {
    const int64_t E = (int64_t)n.size();
    rb::LanePlan p;
    CHECK(rb::lane_plan(n.data(), E, M, p), "E %lld, M %d: refused", (long long)E, M);
    CHECK(p.waves >= 1 && (int64_t)p.lane_row.size() == (int64_t)p.waves * 64, "%d waves, %zu lanes", p.waves,
          p.lane_row.size());
    CHECK((int64_t)p.wave_env0.size() == (int64_t)p.waves + 1, "%zu wave entries for %d waves", p.wave_env0.size(), p.waves);
    if (p.wave_env0.size() != (size_t)p.waves + 1 || p.lane_row.size() != (size_t)p.waves * 64) return p;
    CHECK(p.wave_env0[0] == 0 && p.wave_env0[p.waves] == E, "the waves cover [%d, %d) of %lld", p.wave_env0[0],
          p.wave_env0[p.waves], (long long)E);
    std::vector<int> lanes((size_t)(E * M), 0);     // lanes of each row
    int64_t next_env = 0;                           // the environment the next head lane must hold
    int32_t epw = 0;
    for (int32_t w = 0; w < p.waves; ++w) {
        CHECK(p.wave_env0[w] == next_env, "wave %d starts at environment %d, expected %lld", w, p.wave_env0[w],
              (long long)next_env);
        CHECK(p.wave_env0[w + 1] > p.wave_env0[w], "wave %d is empty", w);
        int lane = 0;
        while (lane < 64 && p.lane_row[(size_t)w * 64 + lane] >= 0) {
            // a head lane: body 0 of the next environment, followed by its bodies in order
            const int32_t row = p.lane_row[(size_t)w * 64 + lane];
            CHECK(row == next_env * M, "wave %d lane %d: row %d, expected the head of environment %lld", w, lane, row,
                  (long long)next_env);
            if (row != next_env * M) return p;
            const int32_t ne = n[(size_t)next_env];
            CHECK(lane + ne <= 64, "environment %lld crosses the end of wave %d", (long long)next_env, w);
            if (lane + ne > 64) return p;
            for (int32_t b = 0; b < ne; ++b) {
                CHECK(p.lane_row[(size_t)w * 64 + lane + b] == row + b, "environment %lld body %d at wave %d lane %d: row %d",
                      (long long)next_env, b, w, lane + b, p.lane_row[(size_t)w * 64 + lane + b]);
                ++lanes[(size_t)(row + b)];
            }
            lane += ne;
            ++next_env;
        }
        CHECK(next_env == p.wave_env0[w + 1], "wave %d ends at environment %lld, the table says %d", w, (long long)next_env,
              p.wave_env0[w + 1]);
        // next-fit: the following environment did not fit
        if (next_env < E) CHECK(lane + n[(size_t)next_env] > 64, "wave %d: environment %lld would have fitted", w, (long long)next_env);
        for (; lane < 64; ++lane)
            CHECK(p.lane_row[(size_t)w * 64 + lane] == -1, "wave %d lane %d: %d after the idle lanes began", w, lane,
                  p.lane_row[(size_t)w * 64 + lane]);
        const int32_t here = p.wave_env0[w + 1] - p.wave_env0[w];
        if (here > epw) epw = here;
    }
    CHECK(next_env == E, "%lld environments placed of %lld", (long long)next_env, (long long)E);
    CHECK(p.epw_max == epw, "epw_max %d, the waves hold at most %d", p.epw_max, epw);
    for (int64_t e = 0; e < E; ++e)
        for (int32_t b = 0; b < M; ++b)
            CHECK(lanes[(size_t)(e * M + b)] == (b < n[(size_t)e] ? 1 : 0), "environment %lld body %d has %d lanes", (long long)e,
                  b, lanes[(size_t)(e * M + b)]);
    if (want_waves >= 0) CHECK(p.waves == want_waves, "%d waves, expected %d", p.waves, want_waves);
    return p;
}

int main() {
    // uniform counts: the fixed mapping, floor(64 / M) environments per wave
    for (int32_t M : {1, 3, 14, 64}) {
        const int32_t epw = 64 / M;
        for (int64_t E : {(int64_t)1, (int64_t)epw, (int64_t)epw + 1, (int64_t)3 * epw + 2}) {
            const rb::LanePlan p = check_plan(std::vector<int32_t>((size_t)E, M), M, (int)((E + epw - 1) / epw));
            for (int32_t w = 0; w < p.waves; ++w) {
                CHECK(p.wave_env0[w] == w * epw, "M %d wave %d starts at %d", M, w, p.wave_env0[w]);
                for (int lane = 0; lane < 64; ++lane) {
                    const int64_t e = (int64_t)w * epw + lane / M;
                    const int32_t want = lane / M < epw && e < E ? (int32_t)(e * M + lane % M) : -1;
                    CHECK(p.lane_row[(size_t)w * 64 + lane] == want, "M %d wave %d lane %d: %d, the fixed mapping has %d", M, w,
                          lane, p.lane_row[(size_t)w * 64 + lane], want);
                }
            }
            CHECK(p.epw_max == (E < epw ? (int32_t)E : epw), "M %d E %lld: epw_max %d", M, (long long)E, p.epw_max);
        }
    }
    // edge cases
    check_plan({33, 33}, 64, 2);                              // neither fits beside the other
    check_plan({64}, 64, 1);
    {
        const rb::LanePlan p = check_plan(std::vector<int32_t>(130, 1), 1, 3);     // 64 + 64 + 2
        CHECK(p.epw_max == 64 && p.lane_row[2 * 64 + 1] == 129 && p.lane_row[2 * 64 + 2] == -1, "the last partial wave");
    }
    check_plan({31, 33, 1, 64, 1}, 64, 4);                    // 31 + 33 fill a wave exactly; 1; 64; 1
    check_plan({5, 8, 1, 1, 7, 8, 8, 8, 8, 8, 3}, 8, 2);      // a last partial wave: 62 lanes, then 3
    {
        // the ensemble of tests/test_gpu_batch_ragged.py: 87 bodies, environments 0..16 in 62 lanes, the rest in 25
        const std::vector<int32_t> n = {1, 2, 3, 2, 4, 6, 2, 3, 4, 4, 6, 8, 2, 3, 4, 3, 5, 7, 1, 2, 3, 2, 4, 6};
        const rb::LanePlan p = check_plan(n, 8, 2);
        CHECK(p.wave_env0.size() == 3 && p.wave_env0[1] == 17 && p.epw_max == 17, "the split of the box ensemble");
        CHECK(p.lane_row[61] == 16 * 8 + 4 && p.lane_row[62] == -1 && p.lane_row[64 + 24] == 23 * 8 + 5 && p.lane_row[64 + 25] == -1,
              "the last lanes of the box ensemble");
    }
    // a sweep of small pseudo-random populations
    uint32_t seed = 12345u;
    for (int round = 0; round < 400; ++round) {
        seed = seed * 1664525u + 1013904223u;
        const int32_t M = 1 + (int32_t)((seed >> 8) % 64);
        seed = seed * 1664525u + 1013904223u;
        const int64_t E = 1 + (int64_t)((seed >> 8) % 40);
        std::vector<int32_t> n((size_t)E);
        for (auto &c : n) {
            seed = seed * 1664525u + 1013904223u;
            c = 1 + (int32_t)((seed >> 8) % (uint32_t)M);
        }
        check_plan(n, M, -1);
    }
    // refusals
    {
        rb::LanePlan p;
        const int32_t zero[] = {3, 0}, over[] = {3, 9}, ok[] = {3, 8};
        CHECK(!rb::lane_plan(zero, 2, 8, p) && p.waves == 0 && p.lane_row.empty(), "a count of 0 is refused");
        CHECK(!rb::lane_plan(over, 2, 8, p), "a count of M + 1 is refused");
        CHECK(!rb::lane_plan(ok, 2, 65, p) && !rb::lane_plan(ok, 0, 8, p) && !rb::lane_plan(nullptr, 2, 8, p), "bad shapes");
        CHECK(rb::lane_plan(ok, 2, 8, p) && p.waves == 1, "a good plan after refusals");
    }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("host_laneplan: ok\n");
    return 0;
}
