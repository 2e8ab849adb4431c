// rb_world_impulses.hpp — the impulse query of a world (rb_query_impulses,
// rb_query_impulses_dev in include/rbhip.h; kernels in rb_world_impulses.hip):
// for the world's current state and the step parameters of the call, what the
// next step does to a range of bodies, contact by contact, as
// rb_batch_impulses defines it for one environment.
//
// It reads what the contact query reads (rb_world_contacts.hpp: the current
// snapshot, the state rows, the constants, the query's own table) and, for the
// solve, the velocities, the applied forces and the step parameters.  It
// writes nothing of the world.
#pragma once
#include "rb_world_contacts.hpp"

namespace rb {

// c: the range, R and the records both queries share (counts, partner, kind,
// dist; pos and frame stay nullptr), and the parameter block: beside what the
// contact query reads, c.sp holds g, dt, e, mu, thr, oriented and xfrc (stride
// S) as a step's block does.  Beside them, of the caller's element type (c.io32):
template <typename T> struct WorldImpulseQuery {
    WorldContactQuery<T> c;
    void *jn;                          // [count][R]; nullptr with R == 0
    void *jt;                          // [count][R][3]
    void *vel;                         // [count][6] (v, w) after gravity, forces and the contacts, or nullptr
    void *net;                         // [count][6] sum of P, sum of r x P over the applied contacts, or nullptr
};

// boxes: the world holds a box (the instance with the box narrowphase)
template <typename T> hipError_t launch_world_impulses(const WorldImpulseQuery<T> &q, bool boxes, hipStream_t s);

}  // namespace rb
