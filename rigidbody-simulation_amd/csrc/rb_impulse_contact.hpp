// rb_impulse_contact.hpp — the step's treatment of one contact with what it
// computes kept, as a function (the sensing step loop of a sampled run,
// rb_batch_sensed.hip).
// impulses_body (rb_batch_impulses.hip) holds the same text in its contact
// lambda and keeps it: moved onto this function its fp64 instances compiled to
// the same registers, its fp32 ones did not (boxes 168 -> 162 and 174 -> 166,
// spheres 112 -> 116 and 116 -> 124, whether the function is force-inlined or
// not and whether it takes the position by value or by reference), and those
// kernels' resources are pinned.
// Device code only.
#pragma once

#include "rb_device.hpp"
#include "rb_internal.hpp"
#include "rb_body.hpp"

namespace rb {

// K2 on one contact of a body (solve_contact, rb_body.hpp) with jn and jt
// returned: the skip rules (collision.py:74, :79-80), the frame flipped for the
// geom1 body under RB_NORMAL_ORIENTED, impulse / apply (rb_device.hpp) with the
// step's LazyInvI on the body's velocity (v, w).  jn and jt come in as 0: a
// skipped or separating contact leaves them, and applies nothing.  An applied
// one adds P = jn n + jt (as apply evaluates it) to net_p and r x P to net_l.
template <typename T>
__device__ __forceinline__ void contact_impulse(const StepParams<T> &sp, const Contact<T> &con, bool self_g1,
                                                const V3<T> &x, T m, T kk, LazyInvI<T> &invI, V3<T> &v, V3<T> &w, T &jn,
                                                V3<T> &jt, V3<T> &net_p, V3<T> &net_l) {
    if (con.dist < T(0) && !(absval(con.dist) < sp.thr)) {      // collision.py:74, :79-80
        const V3<T> nn = (sp.oriented && self_g1) ? V3<T>{-con.frame.x, -con.frame.y, -con.frame.z} : con.frame;
        const V3<T> r = {con.pos.x - x.x, con.pos.y - x.y, con.pos.z - x.z};   // :75
        if (impulse(kk, v, w, r, nn, sp.e, sp.mu, jn, jt)) {
            apply(v, w, m, invI.get(), r, nn, jn, jt);
            const V3<T> P = {jn * nn.x + jt.x, jn * nn.y + jt.y, jn * nn.z + jt.z};   // (as apply evaluates it)
            const V3<T> L = np_cross(r, P);
            net_p = {net_p.x + P.x, net_p.y + P.y, net_p.z + P.z};
            net_l = {net_l.x + L.x, net_l.y + L.y, net_l.z + L.z};
        }
    }
}

}  // namespace rb
