// rb_batch_impulses.hpp — the impulse query of a batch (rb_batch_impulses,
// rb_batch_impulses_dev in include/rbhip.h; kernels in rb_batch_impulses.hip):
// for the batch's current state and the step parameters of the call, what the
// next step does to every body, contact by contact: the contact list of
// rb_batch_contacts, the two return values of compute_collision_impulse_friction
// for each record, the velocity the solve leaves and the body's net contact
// impulse.  A pure function of the state, the parameters and the batch's
// constants: it steps nothing and writes nothing of the batch.
#pragma once
#include "rb_batch_contacts.hpp"
#include "rb_batch_ragged.hpp"
#include "rb_internal.hpp"

namespace rb {

// Where the answers go.  c: the rows of the query and the records both queries
// share (counts, partner, kind, dist; pos and frame stay nullptr), in
// rb_batch_contacts' layout.  Beside them, of the caller's element type (c.io32):
struct ImpulseQuery {
    ContactQuery c;
    void *jn;                          // [n][M][R]; nullptr with R == 0
    void *jt;                          // [n][M][R][3]
    void *vel;                         // [n][M][6] (v, w) after gravity, forces and the contacts, or nullptr
    void *net;                         // [n][M][6] sum of P, sum of r x P over the applied contacts, or nullptr
};

// p: the batch's state, constants, planes, per-environment rows and status,
// and the step parameters of the call (batch_params: dt, e, mu, thr).  pop: the
// batch's population, or all nullptr without one (every environment holds the
// template's M bodies of the template's kinds).  boxes: some body is a box
// among several (the template's p.cs.kind, or pop.kind): the instances that
// hold the box narrowphase.  M <= 64: floor(64 / M) rows per one-wave
// workgroup; else one row per workgroup of 128, 192 or 256 threads.
template <typename T>
hipError_t launch_batch_impulses(const BatchParams<T> &p, const Population &pop, const ImpulseQuery &q, bool boxes,
                                 hipStream_t s);

}  // namespace rb
