// rb_worldplan.hpp — what rb_world_create decides before its first HIP call,
// as a pure function of the scene's counts and the creation-time switches
// (world_plan), the accessors of the layout word it packs (rb_world::group,
// Grid::super) and the byte counts of a world's buffers.  HIP-free
// (tests/host_worldplan.cpp).
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <optional>

#include "rb_tablegeom.hpp"

namespace rb {

// ---- the layout word: group shape bits of x, y, z in nibbles 0-2, the linear
// layout's period bits of x, y, z in nibbles 3-5, bit 24 linear (else a hash
// per group), bits 25-26 log2 of the heads per line.  The kernels read it as
// Grid::super (rb_grid.hpp).
constexpr int32_t GROUP_PERIOD_MASK = 0xfff << 12;
inline int32_t pack_shape(int bx, int by, int bz) { return bx | (by << 4) | (bz << 8); }
inline int shape_bits(int32_t g, int axis) { return (g >> (4 * axis)) & 15; }
inline int shape_bits(int32_t g) { return shape_bits(g, 0) + shape_bits(g, 1) + shape_bits(g, 2); }
inline int period_bits(int32_t g, int axis) { return (g >> (12 + 4 * axis)) & 15; }
inline int period_bits(int32_t g) { return period_bits(g, 0) + period_bits(g, 1) + period_bits(g, 2); }
inline bool layout_linear(int32_t g) { return (g >> 24) & 1; }
inline int heads_field(int32_t g) { return (g >> 25) & 3; }
// the layout without its period (what a table built for one period shares with every other)
inline int32_t layout_key(int32_t g) { return g & ~GROUP_PERIOD_MASK; }
inline int32_t with_period(int32_t g, int lx, int ly, int lz) {
    return layout_key(g) | (lx << 12) | (ly << 16) | (lz << 20);
}
// one more period bit (a table twice the size): in x, then y, then z
inline int32_t period_bump(int32_t g) {
    return g + (period_bits(g, 0) < 15 ? (1 << 12) : period_bits(g, 1) < 15 ? (1 << 16) : (1 << 20));
}

// ---- byte counts of a world's buffers (esz: bytes per real)
inline size_t snap_bytes(int esz, int64_t Npad) { return (size_t)esz * 4 * (size_t)Npad; }     // [Npad] Snap<T>
inline size_t state_bytes(int esz, int64_t S) { return (size_t)esz * 13 * (size_t)S; }         // 13 rows of S
inline size_t consts_bytes(int esz, int64_t Npad) { return (size_t)esz * 8 * (size_t)Npad; }   // 8 rows of Npad
inline size_t line_bytes(int64_t H) { return sizeof(uint32_t) * LINE_WORDS * (size_t)H; }      // a table's lines
inline size_t slot_snapshot_bytes(int esz, int64_t H) { return (size_t)esz * 4 * LINE_WORDS * (size_t)H; }
constexpr size_t spill_bytes = sizeof(uint32_t) * SPILL_LINE_WORDS * SPILL_LINES;
// records per body: 4 per plane, 1 per sphere partner, up to 4 per
// partner in scenes with boxes (oracle/rb_oracle_impl.h contact_stride)
inline int32_t maxrec(int n_planes, bool boxes, int maxp) { return 4 * n_planes + (boxes ? 4 : 1) * maxp; }
// record slots of a rank's S bodies
inline size_t record_slots(int32_t maxrec, int64_t S) { return (size_t)maxrec * (size_t)(S > 0 ? S : 1); }

// ---- the creation-time switches (RBHIP_*), each empty while not set
struct __attribute__((visibility("hidden"))) WorldSwitches {
    std::optional<int64_t> coop_max_bodies, wide_max_bodies, help_max_bodies, tile_min_bodies;
    std::optional<bool> wide_help, help_search, box_optimistic;
    std::optional<int> tile;                  // -1, 0, 1
    std::optional<int> diag_overflow;
    std::optional<int> table_epoch;           // clamped to [1, EPOCH_MAX]
    std::optional<int64_t> contact_stage_bytes, hash_factor, hash_max_bytes;   // only values > 0
    // RBHIP_HASH_GROUP=bx:by:bz[:mode]: the shape when it parsed and fits 12 bits, the mode ('h' unless given)
    bool hash_group_set = false;
    std::optional<int32_t> hash_group_shape;
    char hash_group_mode = 'h';
    struct Period { int l[3]; };
    std::optional<Period> hash_period;        // three numbers in [0, 15]
    std::optional<int> heads_per_line;
    std::optional<int> split;

    static WorldSwitches from_environ() {
        WorldSwitches s;
        if (const char *ev = getenv("RBHIP_COOP_MAX_BODIES")) s.coop_max_bodies = atoll(ev);
        if (const char *ev = getenv("RBHIP_WIDE_MAX_BODIES")) s.wide_max_bodies = atoll(ev);
        if (const char *ev = getenv("RBHIP_HELP_MAX_BODIES")) s.help_max_bodies = atoll(ev);
        if (const char *ev = getenv("RBHIP_WIDE_HELP")) s.wide_help = atoi(ev) != 0;
        if (const char *ev = getenv("RBHIP_HELP_SEARCH")) s.help_search = atoi(ev) != 0;
        if (const char *ev = getenv("RBHIP_TILE")) s.tile = atoi(ev) < 0 ? -1 : atoi(ev) ? 1 : 0;
        if (const char *ev = getenv("RBHIP_TILE_MIN_BODIES")) s.tile_min_bodies = atoll(ev);
        if (const char *ev = getenv("RBHIP_BOX_OPTIMISTIC")) s.box_optimistic = atoi(ev) != 0;
        if (const char *ev = getenv("RBHIP_DIAG_OVERFLOW")) s.diag_overflow = atoi(ev);
        if (const char *ev = getenv("RBHIP_TABLE_EPOCH")) s.table_epoch = std::max(1, std::min(EPOCH_MAX, atoi(ev)));
        if (const char *ev = getenv("RBHIP_CONTACT_STAGE_BYTES"))
            if (atoll(ev) > 0) s.contact_stage_bytes = atoll(ev);
        if (const char *ev = getenv("RBHIP_HASH_FACTOR"))
            if (atoll(ev) > 0) s.hash_factor = atoll(ev);
        if (const char *ev = getenv("RBHIP_HASH_MAX_BYTES"))
            if (atoll(ev) > 0) s.hash_max_bytes = atoll(ev);
        if (const char *ev = getenv("RBHIP_HASH_GROUP")) {
            int bx = 0, by = 0, bz = 0;
            s.hash_group_set = true;
            if (sscanf(ev, "%d:%d:%d:%c", &bx, &by, &bz, &s.hash_group_mode) >= 3 && bx >= 0 && by >= 0 && bz >= 0 && bx + by + bz <= 12)
                s.hash_group_shape = pack_shape(bx, by, bz);
        }
        if (const char *ev = getenv("RBHIP_HASH_PERIOD")) {
            int a = 0, b = 0, c = 0;
            if (sscanf(ev, "%d:%d:%d", &a, &b, &c) == 3 && a >= 0 && b >= 0 && c >= 0 && a <= 15 && b <= 15 && c <= 15)
                s.hash_period = Period{{a, b, c}};
        }
        if (const char *ev = getenv("RBHIP_HEADS_PER_LINE")) s.heads_per_line = atoi(ev);
        if (const char *ev = getenv("RBHIP_SPLIT")) s.split = atoi(ev);
        return s;
    }
};

// the scene's counts a plan depends on
struct WorldCounts {
    int64_t N = 0;             // bodies
    int32_t P = 1, rank = 0;   // ranks, this one
    bool any_box = false;
    int64_t n_spheres = 0;
    int esz = 8;               // bytes per real (the dtype)
    int max_partners = 0;      // the scene's (0: the default 16)
    int n_planes = 0;
};

// what rb_world_create derives before it allocates: a world starts as its plan (rb_host.hpp rb_world)
struct WorldPlan {
    int64_t S = 0, Npad = 0, lo = 0;   // bodies per rank, S x P, this rank's first
    int32_t n_local = 0;               // bodies this rank owns
    int32_t maxp = 16, maxrec = 0;
    // owned bodies up to which the cooperative search is used: above it
    // the wide form (with its helper wave) is faster (19,600: 14.4 vs 12.1
    // us; 16,384: 11.1 vs 11.3, 12,100: 10.4 vs 11.5 the other way;
    // profiles/r03/wide_help/ab_thresh_flat.txt)
    int64_t coop_max = 16384;
    // above coop_max, up to which the wide one-lane form is used; with its
    // helper wave it is at least as fast as the one-lane form at every size
    // measured (131k / 262k equal, 524k 0.116 -> 0.102 ms, 1M 0.236 ->
    // 0.216, 4M 0.876 -> 0.841; profiles/r03/wide_help/ab_large2.txt), so
    // the one-lane form only runs on request (RBHIP_WIDE_MAX_BODIES)
    int64_t wide_max = INT64_MAX;
    // owned bodies up to which the cooperative form runs with a helper wave
    // per workgroup (inv(I_w), gravity and plane contacts off the body
    // lanes' chain): 4k 8.1 -> 7.4 us, 8k 9.6 -> 8.6; 16k 11.0 -> 11.9 the
    // other way (its waves then share SIMDs)
    int64_t help_max = 12288;
    // the wide form with a helper wave per workgroup (inv(I_w), gravity,
    // plane contacts and the state / constant loads off the body wave;
    // A/B steps 261-460, profiles/r03/wide_help_ab.txt): 32k 13.6 -> 12.9
    // us, C3 16.8 -> 16.1, C4 15.4 -> 14.9, C5 (16,384 cubes) 12.1 -> 9.6
    bool wide_help = true;
    // that form with the contact search shared between its two waves: the
    // helper lane of a body searches four of its eight buckets (rb_grid.hpp
    // search_half_wide; RBHIP_HELP_SEARCH)
    bool help_search = true;
    bool boxes = false;            // box-capable step kernels (any box body; sharded worlds exchange orientations)
    int64_t H = 4096;
    int64_t hmax = 4096;           // the table's growth limit (RBHIP_HASH_MAX_BYTES)
    int32_t group = 0;             // Grid::super: the layout word (above)
    bool split = false;            // the split form's partner lists are kept (RBHIP_SPLIT=1)
    bool slot_snapshots = false;   // the tables keep bucket slot snapshots
    int64_t bytes_per_body_step = 0;
    bool box_opt = true;           // RBHIP_BOX_OPTIMISTIC=0: always launch the box kernel
    int32_t diag_overflow = 0;     // RBHIP_DIAG_OVERFLOW=n (tests): the next n guarded chunk checks
                                   // report a bucket overflow (the roll-back / refit / growth path)
    int32_t epoch_max = EPOCH_DEFAULT;   // RBHIP_TABLE_EPOCH; 1: every step rebuilds its next table
    int tile_mode = -1;            // RBHIP_TILE: 0 off, 1 every eligible world, -1 auto (default: >= tile_min_bodies, off after a roll-back)
    int64_t tile_min_bodies = 65537;   // (the hashed forms win up to C3's 65,536 bodies, the tile form above: DESIGN §4.1)
    size_t cq_limit = (size_t)256 << 20;  // RBHIP_CONTACT_STAGE_BYTES
};

inline int64_t next_pow2(int64_t v) {
    int64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

__attribute__((visibility("hidden"))) inline WorldPlan world_plan(const WorldCounts &sc, const WorldSwitches &sw) {
    WorldPlan w;
    const int64_t N = sc.N;
    w.S = (N + sc.P - 1) / sc.P;
    w.Npad = w.S * sc.P;
    w.lo = w.S * sc.rank;
    const int64_t hi = w.lo + w.S < N ? w.lo + w.S : N;
    w.n_local = (int32_t)(hi > w.lo ? hi - w.lo : 0);
    w.maxp = sc.max_partners > 0 ? sc.max_partners : 16;
    const bool any_box = sc.any_box;
    // box-capable kernels (sharded worlds exchange the boxes' orientations)
    w.boxes = any_box;
    w.maxrec = maxrec(sc.n_planes, any_box, w.maxp);
    // worlds with boxes: the cooperative form only up to 4,608 owned bodies
    // (cubes on the incline, per step, helper / plain cooperative / wide:
    // 4,096 8.6 / 10.7 / 11.7 us, 5,184 10.4 / 12.4 / 10.2, 9,216 12.9 /
    // 15.7 / 10.2, 16,384 14.7 (plain) / 12.2; scripts/form_ab.py)
    if (any_box) w.coop_max = 4608;
    // worlds with boxes keep the helper wave without a share of the search
    // (C5, 16,384 cubes: about 20 % slower per step with it;
    // profiles/help_search/shapes_ab.log)
    if (any_box) w.help_search = false;
    if (sw.coop_max_bodies) w.coop_max = *sw.coop_max_bodies;
    if (sw.wide_max_bodies) w.wide_max = *sw.wide_max_bodies;
    if (sw.help_max_bodies) w.help_max = *sw.help_max_bodies;
    if (sw.wide_help) w.wide_help = *sw.wide_help;
    if (sw.help_search) w.help_search = *sw.help_search;
    // the cell-ordered tile form (rb_tiles.hip): RBHIP_TILE = 0 off, 1 every
    // eligible world, -1 auto, the default (eligible worlds of >=
    // RBHIP_TILE_MIN_BODIES bodies, until their first roll-back): it measures
    // slower than the hashed forms up to 65,536 flat spheres (C3) and faster
    // from 73,984 up
    if (sw.tile) w.tile_mode = *sw.tile;
    if (sw.tile_min_bodies) w.tile_min_bodies = *sw.tile_min_bodies;
    if (sw.box_optimistic) w.box_opt = *sw.box_optimistic;
    if (sw.diag_overflow) w.diag_overflow = *sw.diag_overflow;
    if (sw.table_epoch) w.epoch_max = *sw.table_epoch;
    // rb_query_contacts: the bound of its staging buffer
    if (sw.contact_stage_bytes) w.cq_limit = (size_t)*sw.contact_stage_bytes;
    // buckets: cooperative worlds (a hash per cell; they also keep a slot
    // snapshot line per bucket) 16 per body; the one-lane and wide forms
    // (linear cell groups, below) 32 per body, so the groups' period spans
    // the scene (C3: 2^21 buckets, 205 m x 102 m x 12.8 m; as fast as 2^23,
    // 16 per body 20 % slower: the period then folds the scene onto itself).
    // At most 2^26 buckets (8 GB of lines per table).
    const bool coop_world = w.n_local <= w.coop_max;
    int64_t want = coop_world ? 16 * N : 32 * N;
    if (sw.hash_factor) want = *sw.hash_factor * N;
    if (want < 4096) want = 4096;
    // memory cap over both tables (lines, plus slot snapshots in cooperative
    // worlds): RBHIP_HASH_MAX_BYTES, default 8 GiB (1M bodies keep 32 buckets
    // per body, 4M bodies get 8)
    const int64_t per_bucket = 2 * (int64_t)(sizeof(uint32_t) * LINE_WORDS + (coop_world ? sc.esz * 4 * LINE_WORDS : 0));
    int64_t cap_bytes = int64_t(8) << 30;
    if (sw.hash_max_bytes) cap_bytes = *sw.hash_max_bytes;
    int64_t hmax = 4096;
    while (hmax * 2 * per_bucket <= cap_bytes && hmax < (int64_t(1) << 26)) hmax *= 2;
    w.H = next_pow2(want) < hmax ? next_pow2(want) : hmax;
    w.hmax = hmax;
    // The one-lane and wide forms group cells 8x8x4, the buckets of a group
    // contiguous (32 KB of lines), and lay the groups out linearly, periodic
    // in 2^lx x 2^ly x 2^lz groups (below): against a hash per cell measured
    // 6 % faster at 65k bodies (flat), 5 % (incline), 12 % at 1M; hashed
    // groups were bimodal (a group collision doubles the bodies of every
    // bucket in both groups and sends waves through the wide form's extra
    // round trip for buckets of 7+ ids).  Those kernels compute
    // the linear layout directly (rb_grid.hpp LAYOUT_LINEAR), so their worlds
    // always use it.  The cooperative form keeps a hash per cell.
    // RBHIP_HASH_GROUP=bx:by:bz sets the group shape (2^bx x 2^by x 2^bz
    // cells); in cooperative worlds bx:by:bz hashes the groups and
    // bx:by:bz:l lays them out linearly.
    int32_t gshape = coop_world ? 0 : 0x233;
    bool linear = !coop_world;
    if (sw.hash_group_set) {
        if (sw.hash_group_shape) gshape = *sw.hash_group_shape;
        if (coop_world) linear = sw.hash_group_mode == 'l';
    }
    // a table too small for the groups: smaller groups (linear), none (hashed)
    while (gshape && (int64_t(1) << shape_bits(gshape)) > w.H / 4) {
        if (!linear) { gshape = 0; break; }
        for (int sh = 8; sh >= 0; sh -= 4)
            if ((gshape >> sh) & 15) { gshape -= 1 << sh; break; }
    }
    w.group = gshape;
    if (linear) {
        // the group slots split into a period of 2^lx x 2^ly x 2^lz groups (z: at most 8)
        int lg = 0;
        while ((int64_t(1) << (lg + 1)) <= w.H) ++lg;
        lg -= shape_bits(gshape);
        const int lz = lg / 3 < 3 ? lg / 3 : 3, lx = (lg - lz + 1) / 2, ly = lg - lz - lx;
        int l[3] = {lx, ly, lz};
        // diagnostic: RBHIP_HASH_PERIOD=lx:ly:lz sets the creation-time split
        // (at most the table's group bits; with RBHIP_FIT_PERIOD=0 it stays).
        // A zero on an axis whose groups are one cell thick makes a body's
        // two cells along that axis one bucket (tests of the visit-once rule)
        if (sw.hash_period && sw.hash_period->l[0] + sw.hash_period->l[1] + sw.hash_period->l[2] <= lg)
            for (int k = 0; k < 3; ++k) l[k] = sw.hash_period->l[k];
        w.group = with_period(w.group, l[0], l[1], l[2]) | (1 << 24);
    }
    // heads per 128-byte line (rb_internal.hpp Table): 4 in wide-form worlds
    // (C3 17.4 -> 16.4 us), 2 in one-lane worlds (1M 0.237 -> 0.225 ms; 4
    // there cost 10 % at 262k), 1 in cooperative worlds (no gain measured).
    // The cooperative and wide kernels assume theirs at compile time;
    // RBHIP_HEADS_PER_LINE = 1, 2 or 4 sets the one-lane worlds'.
    const bool wide_world = !coop_world && w.n_local <= w.wide_max;
    int rl = coop_world ? 0 : wide_world ? 2 : 1;
    if (sw.heads_per_line && !coop_world && !wide_world) {
        const int r = *sw.heads_per_line;
        if (r == 1 || r == 2 || r == 4) rl = r == 1 ? 0 : r == 2 ? 1 : 2;
    }
    w.group |= rl << 25;
    // algorithmic bytes per body-step: 13 state reals read + 13
    // written + constants (m, I[3], r | h[3])
    const int64_t nsph = sc.n_spheres;
    w.bytes_per_body_step = (int64_t)sc.esz * (26 + 4) + (int64_t)sc.esz * ((nsph * 1 + (N - nsph) * 3) / N);
    // Opt-in (RBHIP_SPLIT=1): large scenes step in two kernels (search,
    // update) joined by a partner list; bit-exact with the oracle on the
    // device (tests/test_gpu_parity.py ragged-scene test) but no faster
    // (DESIGN §5), so the default is the fused one-kernel step.
    w.split = !coop_world && !w.boxes && sw.split && *sw.split == 1;
    // slot snapshots feed the cooperative search only
    w.slot_snapshots = needs_slot_snapshots(coop_world, w.split);
    return w;
}

}  // namespace rb
