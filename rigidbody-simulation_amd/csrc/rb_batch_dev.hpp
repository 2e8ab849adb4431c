// rb_batch_dev.hpp — the device-resident boundary of a batch (rb_batch_*_dev
// in include/rbhip.h; kernels in rb_batch_dev.hip): the caller's arrays are
// device memory, environment-major arrays of structures ([E * M][7] qpos,
// [E * M][6] qvel / xfrc) of doubles or floats, whatever the batch's real type.
#pragma once
#include "rb_internal.hpp"

namespace rb {

constexpr uint32_t DEV_NO_SLOT = 0xffffffffu;   // the refusal word while nothing was refused

// the batch's side of a state transfer
template <typename T> struct DevState {
    Snap<T> *snap;                     // [N]
    BodyState<T> st;                   // rows of N
    const T *bound;                    // [N] bounding radii (set_state writes them into the snapshots)
    int32_t *code;                     // [E]
    int64_t *steps_done;               // [E]
    int64_t N;
    int32_t M;
};

// IO: the element type of the caller's arrays (double / float); conversion is a C cast.
// mask: [E] bytes or nullptr (all); where set, the environment's 13 values and
// snapshot are written and its status and step count cleared (one kernel)
template <typename T, typename IO>
hipError_t launch_dev_state_in(const DevState<T> &p, const uint8_t *mask, const IO *qpos, const IO *qvel, hipStream_t s);
// qpos / qvel: either may be nullptr
template <typename T, typename IO> hipError_t launch_dev_state_out(const DevState<T> &p, IO *qpos, IO *qvel, hipStream_t s);
// applied forces [N][6]: first the check (the smallest slot with a non-finite
// value into *refused by atomic minimum), then the transpose into the rows
// [6][N], which writes nothing while *refused is set
template <typename IO> hipError_t launch_dev_xfrc_check(const IO *xfrc, int64_t N, uint32_t *refused, hipStream_t s);
template <typename T, typename IO>
hipError_t launch_dev_xfrc_in(const IO *xfrc, T *rows, int64_t N, const uint32_t *refused, hipStream_t s);
// slots [0, n) of the sample buffer (rows struct-of-arrays rows of N reals
// each) -> qpos [n][N][7] and (rows == 13) qvel [n][N][6]
template <typename T, typename IO>
hipError_t launch_dev_samples_out(const T *samp, int32_t n, int32_t rows, int64_t N, IO *qpos, IO *qvel, hipStream_t s);

}  // namespace rb
