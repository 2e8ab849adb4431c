// Checks of the two HIP-free host headers (rb_hostpool.hpp, rb_period.hpp),
// compiled as plain host C++ and run by tests/test_host_units.py with
// RBHIP_HOST_THREADS = 1 and 4.  Exit status 0: every check passed.
#include <stdio.h>

#include <thread>

#include "rb_hostpool.hpp"
#include "rb_period.hpp"

using namespace rb::host;

static std::atomic<int> failures{0};
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++failures;                                   \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
        }                                                 \
    } while (0)

// HostPool::run(n, fn) covers [0, n) exactly once: every index is counted by
// the piece that holds it, and the pieces' lengths add up to n.
static void check_cover(size_t n, int caller) {
    std::vector<uint8_t> hits(n, 0);
    std::atomic<size_t> total{0};
    HostPool::get().run(n, [&](size_t lo, size_t hi) {
        if (lo > hi || hi > n) { total += n + 1; return; }
        for (size_t k = lo; k < hi; ++k) ++hits[k];   // (pieces are disjoint: an overlap shows as a count of 2)
        total += hi - lo;
    });
    size_t bad = 0;
    for (size_t k = 0; k < n; ++k) bad += hits[k] != 1;
    CHECK(total.load() == n && bad == 0, "run(%zu) from caller %d: pieces sum to %zu, %zu indices not hit once", n, caller,
          total.load(), bad);
}

static void check_pool() {
    const size_t sizes[] = {0, 1, (1u << 15) - 1, 1u << 15, (1u << 15) + 1, 1000003};
    // two caller threads at once, each over every size (jobs of the two interleave)
    std::thread other([&] { for (int r = 0; r < 3; ++r) for (size_t n : sizes) check_cover(n, 1); });
    for (int r = 0; r < 3; ++r) for (size_t n : sizes) check_cover(n, 0);
    other.join();

    // par_copy2 / par_equal2 against memcpy / memcmp: each array just below
    // and above the 2^15 inline threshold, and the two together (what the
    // pool sees) just below, at and above it
    const size_t pairs[][2] = {{(1u << 15) - 1, (1u << 15) + 1}, {(1u << 15) + 1, (1u << 15) - 1},
                               {(1u << 14) - 1, 1u << 14}, {1u << 14, 1u << 14}, {(1u << 14) + 1, 1u << 14},
                               {1u << 15, 7}, {40000, 50001}, {0, 1u << 15}, {(1u << 15) + 5, 0}};
    for (const auto &pr : pairs) {
        const size_t n0 = pr[0], n1 = pr[1];
        std::vector<double> s0(n0), s1(n1), d0(n0, -1.0), d1(n1, -1.0), m0(n0, -2.0), m1(n1, -2.0);
        for (size_t k = 0; k < n0; ++k) s0[k] = 0.5 * (double)k + 1.0;
        for (size_t k = 0; k < n1; ++k) s1[k] = -0.25 * (double)k - 3.0;
        par_copy2(d0.data(), s0.data(), n0, d1.data(), s1.data(), n1);
        if (n0) memcpy(m0.data(), s0.data(), sizeof(double) * n0);
        if (n1) memcpy(m1.data(), s1.data(), sizeof(double) * n1);
        CHECK((!n0 || memcmp(d0.data(), m0.data(), sizeof(double) * n0) == 0) &&
                  (!n1 || memcmp(d1.data(), m1.data(), sizeof(double) * n1) == 0),
              "par_copy2(%zu, %zu) differs from memcpy", n0, n1);
        CHECK(par_equal2(d0.data(), s0.data(), n0, d1.data(), s1.data(), n1), "par_equal2(%zu, %zu): equal arrays", n0, n1);
        // one differing element at the start, the middle and the end of each array
        for (int a = 0; a < 2; ++a) {
            std::vector<double> &d = a ? d1 : d0;
            const size_t n = a ? n1 : n0;
            if (!n) continue;
            for (size_t at : {size_t(0), n / 2, n - 1}) {
                const double keep = d[at];
                d[at] = keep + 1.0;
                const bool eq = par_equal2(d0.data(), s0.data(), n0, d1.data(), s1.data(), n1);
                const bool ref = (!n0 || memcmp(d0.data(), s0.data(), sizeof(double) * n0) == 0) &&
                                 (!n1 || memcmp(d1.data(), s1.data(), sizeof(double) * n1) == 0);
                CHECK(eq == ref && !eq, "par_equal2(%zu, %zu): array %d differs at %zu", n0, n1, a, at);
                d[at] = keep;
            }
        }
    }
}

// A fixed occupancy set: groups of 8 x 8 x 4 cells (the default shape), one
// body in the first cell of each group; need[] from the cell extents as
// fit_period computes it.
struct Occupancy {
    const char *name;
    std::vector<int64_t> occ;
    int64_t ghi[3];   // (the lowest group is 0 on every axis)
    int lg;
    int expect[3];    // what the functions returned before they moved to rb_period.hpp
};

static void split_of(const Occupancy &o, int lg, int best[3]) {
    const int gb[3] = {3, 3, 2};
    double need[3];
    for (int d = 0; d < 3; ++d) need[d] = double((o.ghi[d] << gb[d]) + 2) / double(1 << gb[d]);
    best_period_split(PeriodSet(o.occ), need, lg, best);
}

static void check_period() {
    Occupancy sheet{"16x16x1 sheet", {}, {15, 15, 0}, 8, {3, 4, 1}};
    for (int x = 0; x < 16; ++x)
        for (int y = 0; y < 16; ++y) sheet.occ.push_back(period_pack(x, y, 0));
    Occupancy block{"4x4x4 block", {}, {3, 3, 3}, 6, {0, 3, 3}};
    for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 4; ++y)
            for (int z = 0; z < 4; ++z) block.occ.push_back(period_pack(x, y, z));
    Occupancy diag{"12-group diagonal", {}, {11, 11, 11}, 5, {1, 2, 2}};
    for (int k = 0; k < 12; ++k) diag.occ.push_back(period_pack(k, k, k));

    for (int64_t g : {int64_t(-5), int64_t(0), int64_t(1) << 19})
        CHECK(period_unpack(period_pack(g, -g, g + 1), 0) == g && period_unpack(period_pack(g, -g, g + 1), 1) == -g &&
                  period_unpack(period_pack(g, -g, g + 1), 2) == g + 1,
              "period_pack / period_unpack round trip at %lld", (long long)g);
    for (const Occupancy *o : {&sheet, &block, &diag}) {
        int best[3] = {-1, -1, -1};
        split_of(*o, o->lg, best);
        CHECK(best[0] == o->expect[0] && best[1] == o->expect[1] && best[2] == o->expect[2],
              "%s, lg %d: split %d %d %d, expected %d %d %d", o->name, o->lg, best[0], best[1], best[2], o->expect[0],
              o->expect[1], o->expect[2]);
        // every lg a table can have (each part holds at most 15 bits)
        for (int lg = 0; lg <= 45; lg += lg < 24 ? 1 : 7) {
            int b[3] = {-1, -1, -1};
            split_of(*o, lg, b);
            CHECK(b[0] + b[1] + b[2] == lg && b[0] >= 0 && b[1] >= 0 && b[2] >= 0 && b[0] <= 15 && b[1] <= 15 && b[2] <= 15,
                  "%s, lg %d: split %d %d %d", o->name, lg, b[0], b[1], b[2]);
        }
    }
}

int main() {
    check_pool();
    check_period();
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures.load());
    return failures ? 1 : 0;
}
