// rb_world_contacts.hpp — the contact query of a world (rb_query_contacts,
// rb_query_contacts_dev in include/rbhip.h; kernels in rb_world_contacts.hip):
// for the world's current state, the contact list of a range of bodies as
// rb_batch_contacts defines it for one environment.
//
// The query reads the current snapshot, the state rows and the constants, and
// a broadphase table of its own (rb_api_contacts.hip: filled by launch_insert
// from the same snapshot under a generation of its own, before the kernel).
// It never reads or writes the tables the steps use, nor the world's error
// word: a body it cannot list is marked in counts and in the query's own
// error word.
#pragma once
#include "rb_internal.hpp"

namespace rb {

constexpr int QUERY_MAXP = 32;           // the partner list of the query's search, whatever the world's max_partners
constexpr int32_t QUERY_NO_LIST = -2;    // counts of a body whose list cannot be built

// Dense arrays, R slots per body: body first + k has counts[k] (the true
// number of contacts, past R too; QUERY_NO_LIST) and the slots [k * R, + R)
// of partner / kind / dist and, times 3, of pos / frame.  Slots at or past
// the count hold kind -1 and zeros elsewhere.
template <typename T> struct WorldContactQuery {
    // what the search and the walk read.  sp.cur: the query's table; sp.next.line
    // null; sp.err: the query's error word; sp.snap_cur, st, cs, grid, planes,
    // n_global: the world's as they stand.  No other field is read.
    StepParams<T> sp;
    int32_t *counts;                   // [count]
    int32_t *partner, *kind;           // [count][R]; nullptr with R == 0
    void *dist;                        // [count][R] reals of the caller's element type
    void *pos, *frame;                 // [count][R][3]; either may be nullptr
    int64_t first, count;              // bodies [first, first + count)
    int32_t R;
    int32_t io32;                      // the caller's element type is float (else double); conversion is a C cast
};

// boxes: the world holds a box (the instance with the box narrowphase)
template <typename T> hipError_t launch_world_contacts(const WorldContactQuery<T> &q, bool boxes, hipStream_t s);

}  // namespace rb
