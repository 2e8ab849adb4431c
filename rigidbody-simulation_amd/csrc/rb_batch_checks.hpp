// rb_batch_checks.hpp — what the launchers of the batch kernels check, once
// (rb_batch_boxes.hip, rb_batch_wide.hip, rb_batch_ragged.hip,
// rb_batch_contacts.hip), and the block of a wide environment as a constant.
// Host code only.
#pragma once

#include <type_traits>
#include "rb_internal.hpp"
#include "rb_batch_contacts.hpp"

namespace rb {

// the sample buffer and the schedule of a recording launch
template <typename T> inline bool rec_ok(const BatchParams<T> &p) {
    return p.samp && p.every >= 1 && p.phase >= 1 && p.phase <= p.every && (p.samp_rows == 7 || p.samp_rows == 13);
}

// a query's outputs and its rows, for environments of M_min..M_max bodies
template <typename T> inline bool query_ok(const BatchParams<T> &p, const ContactQuery &q, int M_min, int M_max) {
    if (p.M < M_min || p.M > M_max || p.n_planes < 0 || p.n_planes > MAX_PLANES || q.R < 0 || !q.counts) return false;
    if (q.R > 0 && (!q.partner || !q.kind || !q.dist)) return false;
    return q.ids || (q.env0 >= 0 && q.env0 + q.n <= p.E);
}

// the block of an environment of 65..256 bodies as a compile-time constant
template <typename F> inline void with_block(int M, F &&f) {
    if (M <= 128) f(std::integral_constant<int, 128>{});
    else if (M <= 192) f(std::integral_constant<int, 192>{});
    else f(std::integral_constant<int, 256>{});
}

}  // namespace rb
