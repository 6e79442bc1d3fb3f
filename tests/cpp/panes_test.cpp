// Host check of the pane arithmetic in flock_amd/csrc/panes.hpp (A-PN1..3, A-PN8) against 128-bit integers: the exact difference, the floor
// division, the threshold of a pane and the Int64 fit.  Stand-alone (tests/test_pane_split_reference.py builds it with the address and
// undefined-behaviour sanitizers and runs it).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "panes.hpp"

using namespace flockgpu::panes;
typedef __int128 i128;

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            if (++failures < 20) {                           \
                printf("FAILED %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);                         \
                printf("\n");                                \
            }                                                \
        }                                                    \
    } while (0)

static i128 floor_div_ref(i128 a, i128 b) {   // b > 0
    i128 q = a / b;
    if (a % b != 0 && a < 0) --q;
    return q;
}
static bool fits(i128 v) { return v >= (i128)INT64_MIN && v <= (i128)INT64_MAX; }

static void check_pane(int64_t t, int64_t origin, int64_t hop) {
    const i128 want = floor_div_ref((i128)t - (i128)origin, (i128)hop);
    const Wide d = exact_diff(t, origin);
    const i128 got_d = d.neg ? -(i128)d.mag : (i128)d.mag;
    CHECK(got_d == (i128)t - (i128)origin, "exact_diff(%lld, %lld)", (long long)t, (long long)origin);
    CHECK(!(d.neg && d.mag == 0), "exact_diff gave -0");
    const Wide p = pane_wide(t, origin, hop);
    const i128 got_p = p.neg ? -(i128)p.mag : (i128)p.mag;
    CHECK(got_p == want, "pane_wide(%lld, %lld, %lld)", (long long)t, (long long)origin, (long long)hop);
    CHECK(!(p.neg && p.mag == 0), "pane_wide gave -0");
    int64_t pane = 12345;
    const bool ok = pane_of(t, origin, hop, &pane);
    CHECK(ok == fits(want), "pane_of fit (%lld, %lld, %lld)", (long long)t, (long long)origin, (long long)hop);
    if (ok) CHECK((i128)pane == want, "pane_of value (%lld, %lld, %lld): %lld", (long long)t, (long long)origin, (long long)hop, (long long)pane);
    else CHECK(pane == 12345, "a refused pane_of wrote its output");
}

static void check_threshold(int64_t p, int64_t origin, int64_t hop) {
    const i128 want = (i128)origin + (i128)p * (i128)hop;
    int64_t thr = 777;
    const bool ok = pane_threshold(p, origin, hop, &thr);
    CHECK(ok == fits(want), "pane_threshold fit (%lld, %lld, %lld)", (long long)p, (long long)origin, (long long)hop);
    if (!ok) return;
    CHECK((i128)thr == want, "pane_threshold value (%lld, %lld, %lld)", (long long)p, (long long)origin, (long long)hop);
    // the round trip: the threshold is the first timestamp of its pane
    int64_t back = 0;
    CHECK(pane_of(thr, origin, hop, &back) && back == p, "pane(threshold(%lld)) with origin %lld hop %lld gave %lld", (long long)p, (long long)origin,
          (long long)hop, (long long)back);
    if (thr > INT64_MIN && p > INT64_MIN) CHECK(pane_of(thr - 1, origin, hop, &back) && back == p - 1, "pane(threshold(%lld) - 1) with origin %lld hop %lld gave %lld",
                                                (long long)p, (long long)origin, (long long)hop, (long long)back);
}

int main() {
    const std::vector<int64_t> hops = {1, 2, 3, 1000, 5000, (int64_t)1 << 31, ((int64_t)1 << 31) + 1, (int64_t)1 << 62, INT64_MAX};
    const std::vector<int64_t> origins = {0, 1, -1, 4999, -4999, 1600000000000ll, -1600000000000ll, INT64_MAX, INT64_MIN, INT64_MAX - 1, INT64_MIN + 1,
                                          (int64_t)1 << 62, -((int64_t)1 << 62)};
    std::vector<int64_t> times = {0, 1, -1, 2, -2, 4999, 5000, 5001, -4999, -5000, -5001, INT64_MAX, INT64_MAX - 1, INT64_MIN, INT64_MIN + 1,
                                  (int64_t)1 << 31, -((int64_t)1 << 31), (int64_t)1 << 62, -((int64_t)1 << 62), 1600000000123ll};
    uint64_t x = 0x9e3779b97f4a7c15ull;   // (xorshift: seeded, reproducible)
    for (int i = 0; i < 2000; ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        times.push_back((int64_t)x >> (i % 40));
    }
    for (int64_t hop : hops)
        for (int64_t origin : origins) {
            for (int64_t t : times) check_pane(t, origin, hop);
            // t = origin - 1 lies in pane -1, t = origin in pane 0 (A-PN1)
            int64_t p = 0;
            if (origin > INT64_MIN) CHECK(pane_of(origin - 1, origin, hop, &p) && p == -1, "origin - 1 is not in pane -1");
            CHECK(pane_of(origin, origin, hop, &p) && p == 0, "origin is not in pane 0");
            // thresholds: around zero, at the ends of what fits, and of the panes of every timestamp above
            for (int64_t q : {(int64_t)0, (int64_t)1, (int64_t)-1, (int64_t)2, (int64_t)-2, (int64_t)65535, (int64_t)-65536, INT64_MAX, INT64_MIN, INT64_MAX / 2, INT64_MIN / 2})
                check_threshold(q, origin, hop);
            for (size_t i = 0; i < times.size(); i += 7) {
                int64_t q = 0;
                if (!pane_of(times[i], origin, hop, &q)) continue;
                check_threshold(q, origin, hop);
                if (q < INT64_MAX) check_threshold(q + 1, origin, hop);
            }
        }
    // the Int64-fit refusal: with hop = 1 the pane id is the difference itself
    int64_t p = 0;
    CHECK(!pane_of(INT64_MAX, -1, 1, &p), "pane 2^63 fits");
    CHECK(!pane_of(INT64_MAX, INT64_MIN, 1, &p), "pane 2^64 - 1 fits");
    CHECK(!pane_of(INT64_MIN, 1, 1, &p), "pane -2^63 - 1 fits");
    CHECK(pane_of(INT64_MIN, 0, 1, &p) && p == INT64_MIN, "pane -2^63 does not fit");
    CHECK(pane_of(INT64_MAX, 0, 1, &p) && p == INT64_MAX, "pane 2^63 - 1 does not fit");
    CHECK(pane_of(INT64_MAX, INT64_MIN, 2, &p) && p == INT64_MAX, "floor((2^64 - 1) / 2) does not fit");
    CHECK(pane_of(INT64_MIN, INT64_MAX, 2, &p) && p == INT64_MIN, "floor(-(2^64 - 1) / 2) does not fit");
    // wide_less orders 65-bit values
    CHECK(wide_less(Wide{5, true}, Wide{4, true}) && !wide_less(Wide{4, true}, Wide{5, true}) && wide_less(Wide{1, true}, Wide{0, false}) &&
              !wide_less(Wide{0, false}, Wide{0, false}) && wide_less(Wide{0, false}, Wide{~uint64_t(0), false}),
          "wide_less");
    if (failures) {
        printf("panes_test: %d FAILED\n", failures);
        return 1;
    }
    printf("panes_test: ok\n");
    return 0;
}
