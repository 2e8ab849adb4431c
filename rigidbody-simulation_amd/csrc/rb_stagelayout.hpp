// rb_stagelayout.hpp — how the host form of a query (rb_query_contacts, rb_query_impulses,
// rb_batch_contacts, rb_batch_impulses) lays its arrays out in the staging
// buffer.  HIP-free: plain host C++ (tests/host_stagelayout.cpp).
//
// A query answers for a run of units (a body of a world, a listed environment
// of a batch) in ranges of as many units as fit the buffer.  A layout is the
// list of the query's arrays in staging order, each with its bytes per unit;
// an array the caller left out is absent and takes no room.  For a range of c
// units the arrays lie back to back in list order, each c units long.  The
// reals are listed first and a real is 8 bytes, so every array of every range
// starts 8-byte aligned.  The caller's own arrays are dense over all units:
// the range that starts at unit `first` lands `first` units into each.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rb {

struct StageLayout {
    static constexpr int MAX_FIELDS = 8;
    int n = 0;
    size_t unit[MAX_FIELDS] = {};      // bytes per unit of each field; 0: absent

    // the next field of the list; returns its index
    int add(size_t bytes_per_unit, bool present = true) {
        unit[n] = present ? bytes_per_unit : 0;
        return n++;
    }
    // bytes one unit takes in the staging buffer
    size_t per() const {
        size_t s = 0;
        for (int f = 0; f < n; ++f) s += unit[f];
        return s;
    }
    // units that fit `limit` bytes
    int64_t fit(size_t limit) const { return (int64_t)(limit / per()); }
    // field f of a range of c units: where it starts in the staging buffer, how long it is
    size_t offset(int f, size_t c) const {
        size_t s = 0;
        for (int g = 0; g < f; ++g) s += unit[g] * c;
        return s;
    }
    size_t bytes(int f, size_t c) const { return unit[f] * c; }
    // where the range that starts at unit `first` lies in the caller's array of field f
    size_t caller(int f, size_t first) const { return unit[f] * first; }
    // field f of a range of c units in the buffer at `base`; nullptr: absent
    char *at(char *base, int f, size_t c) const { return unit[f] ? base + offset(f, c) : nullptr; }
};

// The contact lists of units of `bodies` bodies, R slots per body (a world's
// body: bodies 1; a batch's environment: M).  pos, frame: given by the caller.
enum { SC_DIST, SC_POS, SC_FRAME, SC_COUNTS, SC_PARTNER, SC_KIND, SC_FIELDS };
inline StageLayout stage_contacts(size_t bodies, int32_t R, bool pos, bool frame) {
    const size_t slots = bodies * (size_t)R;
    StageLayout l;
    l.add(sizeof(double) * slots);
    l.add(sizeof(double) * 3 * slots, pos);
    l.add(sizeof(double) * 3 * slots, frame);
    l.add(sizeof(int32_t) * bodies);
    l.add(sizeof(int32_t) * slots);
    l.add(sizeof(int32_t) * slots);
    return l;
}

// The impulse records of environments of M bodies (a world's body: M 1), R
// slots per body.  vel, net: given by the caller.
enum { SI_DIST, SI_JN, SI_JT, SI_VEL, SI_NET, SI_COUNTS, SI_PARTNER, SI_KIND, SI_FIELDS };
inline StageLayout stage_impulses(size_t M, int32_t R, bool vel, bool net) {
    const size_t slots = M * (size_t)R;
    StageLayout l;
    l.add(sizeof(double) * slots);
    l.add(sizeof(double) * slots);
    l.add(sizeof(double) * 3 * slots);
    l.add(sizeof(double) * 6 * M, vel);
    l.add(sizeof(double) * 6 * M, net);
    l.add(sizeof(int32_t) * M);
    l.add(sizeof(int32_t) * slots);
    l.add(sizeof(int32_t) * slots);
    return l;
}

}  // namespace rb
