// rb_batch_sensed.hpp — a sampled run that records contact-impulse curves
// (rb_batch_run_sampled_impulses, rb_batch_run_sampled_impulses_dev in
// include/rbhip.h; kernels in rb_batch_sensed.hip): the step loop of a launch
// with each committed step's net contact impulse (the `net` row of
// rb_batch_impulses for the state the step starts from) summed per body over
// the sampling window, and the sum stored with the sample.
#pragma once
#include "rb_batch_ragged.hpp"
#include "rb_internal.hpp"

namespace rb {

// What a sensing launch reads beside the batch's parameters and population.
// A sample slot is p.samp_rows struct-of-arrays rows of E * M reals: the state
// rows that were asked for (x y z qw qx qy qz, then vx vy vz wx wy wz), then
// the six rows of the window's sum (sum of P, sum of r x P).
struct SensedRun {
    void *acc;                         // [6][E * M] reals: the running window's partial sum, carried across launches
    int32_t box;                       // the template is one box (M == 1; a sphere instance runs it)
    int32_t row_q, row_v, row_net;     // first row of qpos / qvel / net in a slot; row_q, row_v: -1 = not recorded
};

// rows of a slot with these outputs
inline int sensed_rows(bool q, bool v) { return (q ? 7 : 0) + (v ? 6 : 0) + 6; }
inline SensedRun sensed_run(void *acc, bool box, bool q, bool v) {
    return SensedRun{acc, box ? 1 : 0, q ? 0 : -1, v ? (q ? 7 : 0) : -1, sensed_rows(q, v) - 6};
}

// One launch: p.k steps (1..RB_BATCH_CHUNK) with the sampling schedule of a
// recording launch (p.samp, every, phase, samp_first, samp_slots, samp_rows; a
// launch may hold no sample: phase > k).  The fixed E x M mapping of the
// queries: M <= 64 floor(64 / M) environments per one-wave workgroup, else one
// environment per workgroup of 128, 192 or 256 threads; pop: the batch's
// population or all nullptr.  boxes: some body is a box among several.  The
// planes of the workgroup's environments sit in dynamic LDS.
template <typename T>
hipError_t launch_batch_sensed(const BatchParams<T> &p, const Population &pop, const SensedRun &r, bool boxes, hipStream_t s);

// slots [0, n) of the sample buffer -> qpos [n][N][7], qvel [n][N][6], net
// [n][N][6] of the caller's element type (a C cast); qpos and qvel may be
// nullptr, and must be where the slots do not hold their rows
template <typename T, typename IO>
hipError_t launch_sensed_out(const T *samp, int32_t n, int32_t rows, const SensedRun &r, int64_t N, IO *qpos, IO *qvel,
                             IO *net, hipStream_t s);

}  // namespace rb
