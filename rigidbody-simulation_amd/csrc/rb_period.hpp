// rb_period.hpp — the period-split scoring of fit_period (rb_api_state.hip).
// Standard library only: compiles without HIP (tests/host_units.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace rb {
namespace host __attribute__((visibility("hidden"))) {

// Group keys packed 21 bits per axis.
constexpr int64_t PERIOD_OFF = 1 << 20;                  // group coordinates kept in [-2^20, 2^20)
inline int64_t period_pack(int64_t gx, int64_t gy, int64_t gz) {
    return ((gx + PERIOD_OFF) << 42) | ((gy + PERIOD_OFF) << 21) | (gz + PERIOD_OFF);
}
inline int64_t period_unpack(int64_t k, int d) { return ((k >> (42 - 21 * d)) & ((1 << 21) - 1)) - PERIOD_OFF; }
// The groups a search reads (the occupied ones, sorted unique, and their
// neighbours; above 8,192 occupied groups the occupied ones alone), with
// their coordinates and an occupied flag.
struct PeriodSet {
    std::vector<int64_t> qg[3];
    std::vector<uint8_t> qocc;
    explicit PeriodSet(std::vector<int64_t> occ) {
        std::sort(occ.begin(), occ.end());
        occ.erase(std::unique(occ.begin(), occ.end()), occ.end());
        std::vector<int64_t> q;
        q.reserve(occ.size() * 27);
        if (occ.size() > 8192) q = occ;
        else for (int64_t k : occ)
            for (int dz = -1; dz <= 1; ++dz)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx)
                        q.push_back(period_pack(period_unpack(k, 0) + dx, period_unpack(k, 1) + dy, period_unpack(k, 2) + dz));
        std::sort(q.begin(), q.end());
        q.erase(std::unique(q.begin(), q.end()), q.end());
        qocc.resize(q.size());
        for (int d = 0; d < 3; ++d) qg[d].resize(q.size());
        for (size_t t = 0; t < q.size(); ++t) {
            for (int d = 0; d < 3; ++d) qg[d][t] = period_unpack(q[t], d);
            qocc[t] = std::binary_search(occ.begin(), occ.end(), q[t]) ? 1 : 0;
        }
    }
    // groups a search reads that share a run of buckets with another group,
    // at least one of them occupied, under the period 2^l[0] x 2^l[1] x 2^l[2]
    int64_t collisions(const int l[3], std::vector<uint64_t> &f) const {
        f.resize(qocc.size());
        for (size_t t = 0; t < qocc.size(); ++t) {
            uint64_t idx = 0;
            int sh = 0;
            for (int d = 0; d < 3; ++d) {
                idx |= ((uint64_t)qg[d][t] & ((1ull << l[d]) - 1)) << sh;
                sh += l[d];
            }
            f[t] = (idx << 1) | qocc[t];
        }
        std::sort(f.begin(), f.end());
        int64_t coll = 0;
        for (size_t a = 0; a < f.size();) {
            size_t e = a;
            bool any_occ = false;
            while (e < f.size() && (f[e] >> 1) == (f[a] >> 1)) any_occ |= (f[e++] & 1);
            if (any_occ) coll += (int64_t)(e - a) - 1;
            a = e;
        }
        return coll;
    }
};
// The split of lg period bits with the fewest collisions; ties: fewest axes
// the period does not cover (need[d]: groups of extent per axis), then the
// most even cover.
inline void best_period_split(const PeriodSet &ps, const double need[3], int lg, int best[3]) {
    std::vector<uint64_t> f;
    int64_t best_c = -1;
    int best_nf = 0;
    double best_fold = 0.0;
    for (int lx = 0; lx <= lg && lx <= 15; ++lx)
        for (int ly = 0; lx + ly <= lg && ly <= 15; ++ly) {
            const int lz = lg - lx - ly;
            if (lz > 15) continue;
            const int l[3] = {lx, ly, lz};
            const int64_t coll = ps.collisions(l, f);
            double fold = 0.0;
            int nf = 0;                                  // axes the period does not cover
            for (int d = 0; d < 3; ++d) {
                fold = std::max(fold, need[d] / double(1 << l[d]));
                nf += need[d] > double(1 << l[d]);
            }
            if (best_c < 0 || coll < best_c || (coll == best_c && nf < best_nf) ||
                (coll == best_c && nf == best_nf && fold < best_fold - 1e-12)) {
                best_c = coll;
                best_nf = nf;
                best_fold = fold;
                best[0] = lx; best[1] = ly; best[2] = lz;
            }
        }
}

}  // namespace host
}  // namespace rb
