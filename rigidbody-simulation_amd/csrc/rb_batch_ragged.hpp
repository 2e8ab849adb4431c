// rb_batch_ragged.hpp — batches with a population (rb_batch_set_population in
// include/rbhip.h; kernels in rb_batch_ragged.hip): per environment a body
// count n_e in 1..M and a kind for each of its M body slots.  Bodies
// 0..n_e-1 are present, slots n_e..M-1 absent: no step and no query reads or
// writes an absent row.
#pragma once
#include "rb_batch_contacts.hpp"
#include "rb_internal.hpp"

namespace rb {

// What the ragged kernels read beside the batch's parameters.  (A struct of
// its own: BatchParams is the argument block of the kernels of rb_batch.hip,
// rb_batch_boxes.hip, rb_batch_wide.hip and rb_batch_contacts.hip, which stay
// as they are.)
struct Population {
    const int32_t *n_bodies;           // [E] present bodies of each environment
    const int32_t *kind;               // [E * M] the kind of every body slot (read by the BOXES instances only)
    // the lane plan of a one-wave batch (rb_laneplan.hpp; M <= 64)
    const int32_t *wave_env0;          // [waves + 1] a wave's first environment
    const int32_t *lane_row;           // [waves * 64] the lane's row e * M + b, or -1: idle
    int32_t waves;
    int32_t epw_max;                   // most environments of one wave: the stride of the planes block
};

// One launch of the step kernel of a batch with a population: M <= 64
// ragged_step_kernel (lanes packed by the plan), else ragged_wide_kernel (one
// environment per workgroup).  boxes: a present body of some environment is a
// box.  The planes are always read from the wave's LDS block (dynamic LDS:
// epw_max * n_planes * 6 reals, wide: n_planes * 6).
template <typename T>
hipError_t launch_ragged_step(const BatchParams<T> &p, const Population &pop, bool boxes, bool rec, hipStream_t s);
// the contact query (the fixed E x M mapping of rb_batch_contacts.hip / rb_batch_wide.hip)
template <typename T>
hipError_t launch_ragged_contacts(const BatchParams<T> &p, const Population &pop, const ContactQuery &q, bool boxes,
                                  hipStream_t s);

}  // namespace rb
