// cross.hpp's host-callable index helpers against their definitions, on the CPU (plain C++; built with -fsanitize=address,undefined by
// tests/test_plan_cross_join.py): quotient / remainder through the reciprocal against `/` and `%`, the A-X6 limit checks at their edges, and the
// closed-form Utf8 offsets against offsets written out value by value.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cross.hpp"

using namespace flockgpu;

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            if (++fails < 10) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                            \
    } while (0)

int main() {
    // divisors of every class (powers of two, 32-bit and 33-bit multipliers), dividends up to the 2^31 + 15 a kernel can form
    const uint32_t ds[] = {1, 2, 3, 4, 5, 7, 15, 16, 17, 263, 1000, 4095, 4096, 4097, 40003, 70001, 46341, 65535, 65536, 1u << 30, (1u << 31) - 1, 1u << 31, 0x80000001u, 0xffffffffu};
    uint64_t x = 88172645463325252ull;
    for (uint32_t d : ds) {
        const UMod32 m = umod32_make(d);
        auto one = [&](uint32_t n) {
            uint32_t q, r;
            cross_divmod(n, m, &q, &r);
            CHECK(q == n / d && r == n % d);
        };
        for (uint32_t n : {0u, 1u, d - 1, d, d + 1, 2 * d - 1, 2 * d, (1u << 31) - 1, 1u << 31, (1u << 31) + 15, 0xffffffffu}) one(n);
        for (int i = 0; i < 200000; ++i) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            one((uint32_t)x);
        }
    }
    // A-X6
    int64_t n = -1;
    CHECK(cross_rows_ok(46340, 46341, &n) && n == 46340ll * 46341);
    CHECK(!cross_rows_ok(46341, 46341, &n) && n == 0);
    CHECK(cross_rows_ok((1ll << 31) - 1, 1, &n) && n == (1ll << 31) - 1);
    CHECK(!cross_rows_ok(1ll << 31, 1, &n) && !cross_rows_ok(1, 1ll << 31, &n) && !cross_rows_ok(1ll << 62, 1ll << 62, &n) && !cross_rows_ok(INT64_MAX, INT64_MAX, &n));
    CHECK(cross_rows_ok(0, INT64_MAX, &n) && n == 0 && cross_rows_ok(INT64_MAX, 0, &n) && n == 0);
    CHECK(cross_bytes_ok(700000, 3067, &n) && n == 700000ll * 3067 && !cross_bytes_ok(700000, 3068, &n));
    CHECK(cross_bytes_ok(0, INT64_MAX, &n) && n == 0 && !cross_bytes_ok(INT64_MAX, 2, &n));
    // closed-form offsets against offsets written out value by value
    const std::vector<uint32_t> lens = {0, 1, 3, 17, 70, 0, 0, 5, 16, 2};
    std::vector<uint64_t> off(lens.size() + 1, 0);
    for (size_t i = 0; i < lens.size(); ++i) off[i + 1] = off[i] + lens[i];
    const uint64_t total = off.back();
    for (uint32_t times : {1u, 2u, 3u, 16u, 17u}) {
        uint64_t at = 0;   // repeat: value i, `times` times in a row
        for (size_t i = 0; i < lens.size(); ++i)
            for (uint32_t j = 0; j < times; ++j) {
                CHECK(cross_repeat_offset(times, j, off[i], lens[i]) == at);
                at += lens[i];
            }
        CHECK(cross_repeat_offset(times, 0, off[lens.size()], 0) == at && at == total * times);
        at = 0;            // tile: the whole column, `times` times over
        for (uint32_t i = 0; i < times; ++i)
            for (size_t j = 0; j < lens.size(); ++j) {
                CHECK(cross_tile_offset(total, i, off[j]) == at);
                at += lens[j];
            }
        CHECK(cross_tile_offset(total, times, off[0]) == at);
    }
    // the largest products a kernel forms stay inside 64 bits: times * off + j * len with everything just under 2^31
    CHECK(cross_repeat_offset((1ull << 31) - 1, (1u << 31) - 2, (1ull << 31) - 1, (1ull << 31) - 1) == ((1ull << 31) - 1) * ((1ull << 31) - 1) + ((1ull << 31) - 2) * ((1ull << 31) - 1));
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("cross_index_test ok\n");
    return 0;
}
