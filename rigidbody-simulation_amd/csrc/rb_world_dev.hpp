// rb_world_dev.hpp — the device-resident boundary of a world (rb_get_state_dev,
// rb_set_state_dev, rb_set_xfrc_dev in include/rbhip.h; kernels in
// rb_world_dev.hip): the caller's arrays are device memory, arrays of
// structures ([N][7] qpos, [N][6] qvel / xfrc) of doubles or floats, whatever
// the world's real type.  One rank only (a shard's boundary is rb_gpos_buffer).
#pragma once
#include "rb_internal.hpp"

namespace rb {

// the world's side of a state transfer
template <typename T> struct WDevState {
    Snap<T> *snap;                     // the current snapshot (every body)
    T *quat;                           // box worlds: the current orientation snapshot [N][4], else nullptr
    BodyState<T> st;                   // rows of S
    const T *bound;                    // [Npad] bounding radii (the snapshots' fourth word)
    int64_t N;
    int32_t balls;                     // two-ball law: positions are read from the state's px py pz (StateIO)
};

// IO: the element type of the caller's arrays (double / float); conversion is a C cast.
// qpos, qvel -> the 13 state rows, the snapshot and (box worlds) its orientations
template <typename T, typename IO>
hipError_t launch_wdev_state_in(const WDevState<T> &p, const IO *qpos, const IO *qvel, hipStream_t s);
// qpos / qvel: either may be nullptr
template <typename T, typename IO> hipError_t launch_wdev_state_out(const WDevState<T> &p, IO *qpos, IO *qvel, hipStream_t s);
// applied forces [N][6] -> the force rows [6][S] (rows [N, S) are left alone)
template <typename T, typename IO>
hipError_t launch_wdev_xfrc_in(const IO *xfrc, T *rows, int64_t N, int64_t S, hipStream_t s);

}  // namespace rb
