// The staging layouts of the host-form queries (csrc/rb_stagelayout.hpp) as
// plain host C++: the three layouts (a world's contact lists per body, a
// batch's contact lists and impulse records per environment) take the bytes
// per unit their entry points document, lay their arrays out back to back
// without overlap, the reals 8-byte aligned, and cut the caller's arrays into
// consecutive ranges without gap or overlap.  Exit status 0: all checks passed.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "rb_stagelayout.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            ++failures;                                           \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                         \
            fprintf(stderr, "\n");                                \
        }                                                         \
    } while (0)

// l: a layout whose first `reals` fields are reals; present[f]: field f was
// given; per: the closed form of its bytes per unit
static void check_layout(const char *what, const rb::StageLayout &l, int fields, int reals, const bool *present, size_t per) {
    CHECK(l.n == fields, "%s: %d fields", what, l.n);
    CHECK(l.per() == per, "%s: per %zu, closed form %zu", what, l.per(), per);
    for (int f = 0; f < l.n; ++f)
        if (!present[f]) CHECK(l.unit[f] == 0, "%s: absent field %d takes %zu bytes per unit", what, f, l.unit[f]);
    const size_t limits[] = {per - 1, per, 2 * per, 2 * per + 1, 5 * per + per / 2, (size_t)256 << 20};
    for (size_t limit : limits)
        CHECK(l.fit(limit) == (int64_t)(limit / per), "%s: fit(%zu) = %lld", what, limit, (long long)l.fit(limit));
    const size_t ranges[] = {1, 2, 5};
    for (size_t c : ranges) {
        // back to back in list order: no overlap, no gap, the last field ends at c * per
        size_t end = 0;
        std::vector<char> buffer(c * per);
        char *base = buffer.data();
        for (int f = 0; f < l.n; ++f) {
            CHECK(l.offset(f, c) == end, "%s, c %zu: field %d at %zu, the one before ends at %zu", what, c, f, l.offset(f, c), end);
            CHECK(l.bytes(f, c) == c * l.unit[f], "%s, c %zu: field %d is %zu bytes", what, c, f, l.bytes(f, c));
            if (!present[f]) CHECK(l.bytes(f, c) == 0 && l.at(base, f, c) == nullptr, "%s, c %zu: absent field %d", what, c, f);
            if (l.unit[f]) CHECK(l.at(base, f, c) == base + l.offset(f, c), "%s, c %zu: field %d pointer", what, c, f);
            if (f < reals) CHECK(l.offset(f, c) % 8 == 0, "%s, c %zu: real field %d at %zu", what, c, f, l.offset(f, c));
            end = l.offset(f, c) + l.bytes(f, c);
        }
        CHECK(end == c * per, "%s, c %zu: the last field ends at %zu, c * per is %zu", what, c, end, c * per);
        // consecutive ranges of c units (the last one shorter) tile the caller's array of 11 units
        const size_t total = 11;
        for (int f = 0; f < l.n; ++f) {
            size_t covered = 0;
            for (size_t first = 0; first < total; first += c) {
                const size_t cc = total - first < c ? total - first : c;
                CHECK(l.caller(f, first) == covered, "%s, c %zu: field %d range at unit %zu starts at %zu, expected %zu", what,
                      c, f, first, l.caller(f, first), covered);
                covered = l.caller(f, first) + l.bytes(f, cc);
            }
            CHECK(covered == total * l.unit[f], "%s, c %zu: field %d covered %zu of %zu bytes", what, c, f, covered,
                  total * l.unit[f]);
        }
    }
}

int main() {
    const int32_t Rs[] = {0, 1, 4};
    const size_t Ms[] = {1, 4};
    for (int32_t R : Rs)
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) {
                // rb_query_contacts: per body
                {
                    const bool present[] = {R > 0, R > 0 && a, R > 0 && b, true, R > 0, R > 0};
                    const size_t per = sizeof(double) * (size_t)R * (1 + (a ? 3 : 0) + (b ? 3 : 0)) + sizeof(int32_t) * (1 + 2 * (size_t)R);
                    check_layout("world contacts", rb::stage_contacts(1, R, a, b), rb::SC_FIELDS, 3, present, per);
                }
                for (size_t M : Ms) {
                    const size_t MR = M * (size_t)R;
                    // rb_batch_contacts: per listed environment
                    {
                        const bool present[] = {R > 0, R > 0 && a, R > 0 && b, true, R > 0, R > 0};
                        const size_t per = sizeof(double) * MR * (1 + (a ? 3 : 0) + (b ? 3 : 0)) + sizeof(int32_t) * (M + 2 * MR);
                        check_layout("batch contacts", rb::stage_contacts(M, R, a, b), rb::SC_FIELDS, 3, present, per);
                    }
                    // rb_batch_impulses: per listed environment (a: vel, b: net)
                    {
                        const bool present[] = {R > 0, R > 0, R > 0, a != 0, b != 0, true, R > 0, R > 0};
                        const size_t per = sizeof(double) * (5 * MR + (a ? 6 * M : 0) + (b ? 6 * M : 0)) + sizeof(int32_t) * (M + 2 * MR);
                        check_layout("batch impulses", rb::stage_impulses(M, R, a, b), rb::SI_FIELDS, 5, present, per);
                    }
                }
            }
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("host_stagelayout: ok\n");
    return 0;
}
