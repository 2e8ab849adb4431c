// rb_batch_contacts.hpp — the contact query of a batch (rb_batch_contacts,
// rb_batch_contacts_dev in include/rbhip.h; kernels in rb_batch_contacts.hip):
// for the batch's current state, every body's contact list as mj_forward
// generates it for the environment's scene, in the canonical per-body order
// the step kernels walk.  A pure function of the state and the batch's
// constants: it steps nothing and writes nothing of the batch.
#pragma once
#include "rb_internal.hpp"

namespace rb {

// Where the lists go: dense arrays, row t = one listed environment, R slots
// per body.  Body b of row t: counts[t * M + b] (the true number of contacts,
// past R too; -1 for every body of a failed environment) and the slots
// [(t * M + b) * R, + R) of partner / kind / dist and, times 3, of pos /
// frame.  Slots at or past the count hold kind -1 and zeros elsewhere.
struct ContactQuery {
    int32_t *counts;                   // [n][M]
    int32_t *partner, *kind;           // [n][M][R]; nullptr with R == 0
    void *dist;                        // [n][M][R] reals of the caller's element type
    void *pos, *frame;                 // [n][M][R][3]; either may be nullptr
    const int64_t *ids;                // [n] the environment of each row, or nullptr: env0 + row
    int64_t env0, n;
    int32_t R;
    int32_t io32;                      // the caller's element type is float (else double); conversion is a C cast
    int32_t box;                       // the template is one box (M == 1); read by the plain instance only
};

// p: the batch's state, constants, planes and status (batch_params; the step
// constants are not read).  mixed: the template mixes spheres and boxes
// (p.cs.kind: its M kinds), the instance that holds the box narrowphase.
template <typename T>
hipError_t launch_batch_contacts(const BatchParams<T> &p, const ContactQuery &q, bool mixed, hipStream_t s);
// the same for an environment of more than BATCH_BLOCK bodies (rb_batch_wide.hip:
// one row per workgroup); boxes: the template holds a box
template <typename T>
hipError_t launch_batch_wide_contacts(const BatchParams<T> &p, const ContactQuery &q, bool boxes, hipStream_t s);

}  // namespace rb
