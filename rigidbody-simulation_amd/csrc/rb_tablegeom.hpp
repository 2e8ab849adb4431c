// rb_tablegeom.hpp — the broadphase table's geometry constants: what the host's
// world plan (rb_worldplan.hpp) shares with the kernels.  HIP-free;
// rb_internal.hpp includes it and describes the table they measure.
#pragma once

#include <stdint.h>

namespace rb {

constexpr int LINE_WORDS = 32;               // uint32 words per bucket (head + further ids)
constexpr int HEAD_WORDS = 2;                // the header's words
constexpr int BUCKET_SLOTS = LINE_WORDS - HEAD_WORDS;

// A bucket holds 30 ids; a cell with more (a pile-up: C4's sliding rows
// reach 29 by step 700) spills the rest into its table's spill lines: the
// line of the bucket's hash, or the next ones while it is full.  A search
// reads a bucket's spill line(s) only when its count passed its slots.
constexpr int SPILL_LINE_WORDS = 32;
constexpr int SPILL_PAIRS = (SPILL_LINE_WORDS - 2) / 2;   // 15 per line
constexpr int SPILL_LINES = 4096;                         // 512 KB per table
constexpr int SPILL_PROBES = 64;                          // lines tried from the hashed one (<= 960 ids of a bucket)
constexpr int SPILL_GROUP = 1;                            // lines a scan reads per round trip

// append epochs (rb_internal.hpp Epoch)
constexpr int EPOCH_MAX = 64;                // largest RBHIP_TABLE_EPOCH
constexpr int EPOCH_DEFAULT = 8;             // (the measured choice)

// lanes per body of the split form's search kernel (1, or 8 = the
// cooperative search, which reads the bucket slot snapshots)
#ifndef RB_SPLIT_G
#define RB_SPLIT_G 1
#endif
constexpr int SPLIT_SEARCH_LANES = RB_SPLIT_G;

// does a world stepping with these forms need bucket slot snapshots?
inline bool needs_slot_snapshots(bool coop, bool split) { return coop || (split && SPLIT_SEARCH_LANES > 1); }

}  // namespace rb
