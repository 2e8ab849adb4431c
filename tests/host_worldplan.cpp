// host_worldplan.cpp — stand-alone checks of csrc/rb_worldplan.hpp (no HIP, no
// GPU): hand-computed plans taken from the comments the code carries,
// properties over a sweep of scenes, the layout word's accessors, the byte
// counts in their closed forms, and the rows recorded on the device before
// the plan was factored out (one per line on stdin; tests/test_host_worldplan.py).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "rb_worldplan.hpp"

using namespace rb;

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static const char *const SWITCHES[] = {"RBHIP_COOP_MAX_BODIES", "RBHIP_WIDE_MAX_BODIES", "RBHIP_HELP_MAX_BODIES", "RBHIP_WIDE_HELP",
                                       "RBHIP_HELP_SEARCH", "RBHIP_TILE", "RBHIP_TILE_MIN_BODIES", "RBHIP_BOX_OPTIMISTIC",
                                       "RBHIP_DIAG_OVERFLOW", "RBHIP_TABLE_EPOCH", "RBHIP_CONTACT_STAGE_BYTES", "RBHIP_HASH_FACTOR",
                                       "RBHIP_HASH_MAX_BYTES", "RBHIP_HASH_GROUP", "RBHIP_HASH_PERIOD", "RBHIP_HEADS_PER_LINE", "RBHIP_SPLIT"};

// the switches of an environment holding exactly these "KEY=VALUE" settings
static WorldSwitches switches(const std::vector<std::string> &env) {
    for (const char *k : SWITCHES) unsetenv(k);
    for (const std::string &kv : env) {
        const size_t eq = kv.find('=');
        setenv(kv.substr(0, eq).c_str(), kv.substr(eq + 1).c_str(), 1);
    }
    return WorldSwitches::from_environ();
}

static WorldCounts spheres(int64_t N, int esz = 8, int P = 1, int rank = 0) {
    WorldCounts c;
    c.N = N; c.P = P; c.rank = rank; c.n_spheres = N; c.esz = esz; c.n_planes = 1;
    return c;
}
static WorldCounts boxes(int64_t N, int esz = 8, int P = 1, int rank = 0) {
    WorldCounts c = spheres(N, esz, P, rank);
    c.any_box = true; c.n_spheres = 0;
    return c;
}
static int log2i(int64_t v) {
    int l = 0;
    while ((int64_t(1) << (l + 1)) <= v) ++l;
    return l;
}
// the hashed-cell form (include/rbhip.h RB_STAT_FORM: 0 one-lane, 1 cooperative, 2 wide, 3 cooperative + helper, 4 wide + helper)
static int form_of(const WorldPlan &p) {
    return p.n_local <= p.coop_max ? (p.n_local <= p.help_max ? 3 : 1) : p.n_local <= p.wide_max ? (p.wide_help ? 4 : 2) : 0;
}

static void hand_cases() {
    const std::vector<std::string> wide = {"RBHIP_COOP_MAX_BODIES=0"}, one = {"RBHIP_COOP_MAX_BODIES=0", "RBHIP_WIDE_MAX_BODIES=0"};
    auto with = [](std::vector<std::string> v, const char *kv) { v.push_back(kv); return v; };
    {   // 65,536 spheres, the wide form: 32 buckets per body, groups of 8x8x4 cells laid out linearly, 4 heads per line
        const WorldPlan p = world_plan(spheres(65536), switches({}));
        CHECK(form_of(p) == 4 && p.help_search);
        CHECK(p.H == int64_t(1) << 21);
        CHECK((p.group & 0xfff) == 0x233 && layout_linear(p.group) && heads_field(p.group) == 2);
        CHECK(period_bits(p.group, 0) == 5 && period_bits(p.group, 1) == 5 && period_bits(p.group, 2) == 3);
        CHECK(!p.slot_snapshots && !p.split && p.maxp == 16 && p.maxrec == 4 + 16 && p.epoch_max == 8);
        CHECK(p.tile_mode == -1 && p.tile_min_bodies == 65537 && p.box_opt && p.diag_overflow == 0 && p.cq_limit == (size_t)256 << 20);
        CHECK(p.bytes_per_body_step == 8 * 31);
    }
    {   // a cooperative world of 5,000: 16 buckets per body, a hash per cell
        const WorldPlan p = world_plan(spheres(5000), switches({}));
        CHECK(form_of(p) == 3);
        CHECK(p.H == 131072 && p.H == next_pow2(16 * 5000));
        CHECK(p.group == 0 && p.slot_snapshots);
    }
    CHECK(world_plan(spheres(1), switches({})).H == 4096);   // the floor
    {   // 5,000 boxes: past the box worlds' cooperative limit of 4,608
        WorldCounts c = boxes(5000);
        c.n_planes = 3;
        const WorldPlan p = world_plan(c, switches({}));
        CHECK(p.coop_max == 4608 && form_of(p) == 4 && !p.help_search && p.boxes);
        CHECK(p.maxrec == 4 * 3 + 4 * p.maxp);
        CHECK(p.bytes_per_body_step == 8 * 33);
        CHECK(form_of(world_plan(boxes(4000), switches({}))) == 3);
    }
    {   // 4M fp64 bodies under the default 8 GiB cap: 8 buckets per body
        const WorldPlan p = world_plan(spheres(int64_t(1) << 22), switches({}));
        CHECK(p.H == 8 * (int64_t(1) << 22) && p.hmax == p.H);
        CHECK(world_plan(spheres(int64_t(1) << 20), switches({})).H == 32 * (int64_t(1) << 20));
    }
    {   // RBHIP_HASH_GROUP=4:4:4 in a table of 4,096 buckets: at most 1,024 groups' worth of cells per group
        const WorldPlan l = world_plan(spheres(100), switches({"RBHIP_HASH_GROUP=4:4:4:l"}));
        CHECK(l.H == 4096 && (l.group & 0xfff) == 0x244 && layout_linear(l.group));
        CHECK(period_bits(l.group) == 2);
        const WorldPlan h = world_plan(spheres(100), switches({"RBHIP_HASH_GROUP=4:4:4"}));
        CHECK(h.group == 0);
        const WorldPlan k = world_plan(spheres(5000), switches({"RBHIP_HASH_GROUP=2:2:1"}));
        CHECK(k.group == 0x122);
        CHECK(world_plan(spheres(5000), switches({"RBHIP_HASH_GROUP=7:7:7"})).group == 0);   // (more than 12 bits: refused)
    }
    {   // RBHIP_HASH_PERIOD: at most the table's group bits (2^18 buckets, 8 shape bits: 10)
        const WorldPlan a = world_plan(spheres(5000), switches(with(wide, "RBHIP_HASH_PERIOD=3:2:1")));
        CHECK(a.H == int64_t(1) << 18);
        CHECK(period_bits(a.group, 0) == 3 && period_bits(a.group, 1) == 2 && period_bits(a.group, 2) == 1);
        const WorldPlan r = world_plan(spheres(5000), switches(with(wide, "RBHIP_HASH_PERIOD=15:15:15")));
        CHECK(period_bits(r.group, 0) == 4 && period_bits(r.group, 1) == 3 && period_bits(r.group, 2) == 3);
        CHECK(r.group == world_plan(spheres(5000), switches(wide)).group);
    }
    {   // RBHIP_HEADS_PER_LINE: the one-lane worlds' only
        CHECK(heads_field(world_plan(spheres(5000), switches(with(wide, "RBHIP_HEADS_PER_LINE=1"))).group) == 2);
        CHECK(heads_field(world_plan(spheres(5000), switches({"RBHIP_HEADS_PER_LINE=4"})).group) == 0);
        CHECK(heads_field(world_plan(spheres(5000), switches(one)).group) == 1);
        CHECK(heads_field(world_plan(spheres(5000), switches(with(one, "RBHIP_HEADS_PER_LINE=1"))).group) == 0);
        CHECK(heads_field(world_plan(spheres(5000), switches(with(one, "RBHIP_HEADS_PER_LINE=2"))).group) == 1);
        CHECK(heads_field(world_plan(spheres(5000), switches(with(one, "RBHIP_HEADS_PER_LINE=4"))).group) == 2);
        CHECK(heads_field(world_plan(spheres(5000), switches(with(one, "RBHIP_HEADS_PER_LINE=3"))).group) == 1);
        CHECK(form_of(world_plan(spheres(5000), switches(one))) == 0);
    }
    CHECK(world_plan(spheres(100), switches({"RBHIP_TABLE_EPOCH=0"})).epoch_max == 1);
    CHECK(world_plan(spheres(100), switches({"RBHIP_TABLE_EPOCH=100"})).epoch_max == 64);
    CHECK(world_plan(spheres(100), switches({"RBHIP_TABLE_EPOCH=5"})).epoch_max == 5);
    {   // three ranks, ten bodies
        const WorldPlan p = world_plan(spheres(10, 8, 3, 2), switches({}));
        CHECK(p.S == 4 && p.Npad == 12 && p.lo == 8 && p.n_local == 2);
        CHECK(world_plan(spheres(10, 8, 3, 0), switches({})).n_local == 4);
    }
    {   // the other switches
        const WorldPlan p = world_plan(spheres(40000), switches({"RBHIP_SPLIT=1", "RBHIP_TILE=-3", "RBHIP_TILE_MIN_BODIES=7", "RBHIP_BOX_OPTIMISTIC=0",
                                                                  "RBHIP_DIAG_OVERFLOW=2", "RBHIP_CONTACT_STAGE_BYTES=4096", "RBHIP_WIDE_HELP=0",
                                                                  "RBHIP_HELP_SEARCH=0", "RBHIP_HASH_FACTOR=4"}));
        CHECK(p.split && !p.slot_snapshots && p.tile_mode == -1 && p.tile_min_bodies == 7 && !p.box_opt && p.diag_overflow == 2);
        CHECK(p.cq_limit == 4096 && form_of(p) == 2 && !p.help_search && p.H == next_pow2(4 * 40000));
        CHECK(!world_plan(spheres(5000), switches({"RBHIP_SPLIT=1"})).split);    // (cooperative worlds have no split form)
        CHECK(!world_plan(boxes(40000), switches({"RBHIP_SPLIT=1"})).split);     // (nor box worlds)
        CHECK(world_plan(spheres(100), switches({"RBHIP_CONTACT_STAGE_BYTES=-1"})).cq_limit == (size_t)256 << 20);
        CHECK(form_of(world_plan(spheres(16000), switches({}))) == 1);           // (past the helper's 12,288)
        CHECK(form_of(world_plan(spheres(16000), switches({"RBHIP_HELP_MAX_BODIES=16000"}))) == 3);
    }
}

static void layout_word() {
    for (int lx = 0; lx <= 15; ++lx)
        for (int ly = 0; ly <= 15; ++ly)
            for (int lz = 0; lz <= 15; ++lz) {
                const int32_t g = with_period(0x233 | (1 << 24) | (2 << 25), lx, ly, lz);
                CHECK(period_bits(g, 0) == lx && period_bits(g, 1) == ly && period_bits(g, 2) == lz);
                CHECK(layout_key(g) == (0x233 | (1 << 24) | (2 << 25)));
                if (lx + ly + lz == 45) continue;
                // one more bit: in x, then y, then z; nothing else moves
                const int32_t b = period_bump(g);
                CHECK(period_bits(b) == period_bits(g) + 1 && layout_key(b) == layout_key(g));
                CHECK(period_bits(b, 0) == (lx < 15 ? lx + 1 : lx));
                CHECK(period_bits(b, 1) == (lx == 15 && ly < 15 ? ly + 1 : ly));
                CHECK(period_bits(b, 2) == (lx == 15 && ly == 15 ? lz + 1 : lz));
            }
    // exactly the twelve period bits
    CHECK(layout_key(0x7ffffff) == 0x7000fff && layout_key(0x0fff000) == 0);
    CHECK(shape_bits(0x233, 0) == 3 && shape_bits(0x233, 1) == 3 && shape_bits(0x233, 2) == 2 && shape_bits(0x233) == 8);
    CHECK(pack_shape(3, 3, 2) == 0x233);
}

static void sweep() {
    std::vector<int64_t> Ns = {1};
    for (int k = 1; k <= 22; ++k)
        for (int64_t n : {(int64_t(1) << k) - 1, int64_t(1) << k, (int64_t(1) << k) + 1})
            if (n > 1 && n <= (int64_t(1) << 22)) Ns.push_back(n);
    int64_t cases = 0;
    for (int64_t N : Ns)
        for (int esz : {8, 4})
            for (int box = 0; box < 2; ++box)
                for (int P : {1, 2, 8})
                    for (int rank : {0, P - 1}) {
                        const WorldCounts c = box ? boxes(N, esz, P, rank) : spheres(N, esz, P, rank);
                        const WorldPlan p = world_plan(c, switches({}));
                        ++cases;
                        CHECK(p.H >= 4096 && p.H <= p.hmax && (p.H & (p.H - 1)) == 0);
                        CHECK((int64_t(1) << shape_bits(p.group)) <= p.H / 4);
                        if (layout_linear(p.group)) {
                            CHECK(period_bits(p.group) + shape_bits(p.group) == log2i(p.H));
                            CHECK(period_bits(p.group, 2) <= 3);
                        } else {
                            CHECK(period_bits(p.group) == 0);
                        }
                        CHECK(p.S * P >= N && (p.S - 1) * P < N && p.Npad == p.S * P && p.lo == p.S * rank);
                        CHECK(p.n_local == std::max<int64_t>(0, std::min(N, p.lo + p.S) - p.lo));
                        // the byte counts in their closed forms
                        CHECK(snap_bytes(esz, p.Npad) == (size_t)esz * 4 * p.Npad);
                        CHECK(state_bytes(esz, p.S) == (size_t)esz * 13 * p.S);
                        CHECK(consts_bytes(esz, p.Npad) == (size_t)esz * 8 * p.Npad);
                        CHECK(line_bytes(p.H) == (size_t)128 * p.H);
                        CHECK(slot_snapshot_bytes(esz, p.H) == (size_t)esz * 128 * p.H);
                        CHECK(record_slots(p.maxrec, p.S) == (size_t)p.maxrec * p.S);
                        CHECK(p.maxrec == maxrec(c.n_planes, c.any_box, p.maxp) && p.maxrec == 4 + (box ? 64 : 16));
                        // both tables within the cap, unless at the floor
                        const size_t tables = 2 * (line_bytes(p.H) + (p.slot_snapshots ? slot_snapshot_bytes(esz, p.H) : 0));
                        CHECK(p.H == 4096 || tables <= (size_t)8 << 30);
                    }
    CHECK(spill_bytes == (size_t)512 << 10);
    CHECK(record_slots(20, 0) == 20);
    printf("host_worldplan: %lld plans swept\n", (long long)cases);
}

// a recorded row: N P rank any_box n_spheres esz max_partners n_planes, then
// buckets max_partners grid_layout hashed_form help_search table_epoch n_owned
// bytes_per_body_step, whether grid_layout's period is the creation-time one,
// then the switches as KEY=VALUE
static int rows_from_stdin() {
    char line[4096];
    int n = 0;
    while (fgets(line, sizeof line, stdin)) {
        std::vector<std::string> tok;
        for (char *t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) tok.push_back(t);
        if (tok.empty()) continue;
        if (tok.size() < 17) { printf("FAILED: short row\n"); ++failures; continue; }
        long long v[17];
        for (int k = 0; k < 17; ++k) v[k] = atoll(tok[(size_t)k].c_str());
        WorldCounts c;
        c.N = v[0]; c.P = (int32_t)v[1]; c.rank = (int32_t)v[2]; c.any_box = v[3] != 0; c.n_spheres = v[4];
        c.esz = (int)v[5]; c.max_partners = (int)v[6]; c.n_planes = (int)v[7];
        const WorldPlan p = world_plan(c, switches(std::vector<std::string>(tok.begin() + 17, tok.end())));
        const int form = form_of(p);
        const bool ok = p.H == v[8] && p.maxp == v[9] &&
                        (v[16] ? p.group == (int32_t)v[10] : layout_key(p.group) == layout_key((int32_t)v[10])) &&
                        period_bits(p.group) == period_bits((int32_t)v[10]) && form == v[11] &&
                        (form == 4 && p.help_search) == (v[12] != 0) && p.epoch_max == v[13] && p.n_local == v[14] &&
                        p.bytes_per_body_step == v[15];
        if (!ok) {
            printf("FAILED row %d: plan H %lld maxp %d group 0x%x form %d help_search %d epoch %d n_local %d bytes %lld\n", n,
                   (long long)p.H, p.maxp, (unsigned)p.group, form, (int)p.help_search, p.epoch_max, p.n_local,
                   (long long)p.bytes_per_body_step);
            ++failures;
        }
        ++n;
    }
    return n;
}

int main(int argc, char **argv) {
    hand_cases();
    layout_word();
    sweep();
    const int rows = rows_from_stdin();
    if (argc > 1 && rows != atoi(argv[1])) { printf("FAILED: %d rows read, %s expected\n", rows, argv[1]); ++failures; }
    printf("host_worldplan: %d recorded rows\n", rows);
    if (failures) return 1;
    printf("host_worldplan: ok\n");
    return 0;
}
