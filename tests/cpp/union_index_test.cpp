// union.hpp's host-callable index helpers against their definitions, on the CPU (plain C++; built with -fsanitize=address,undefined by
// tests/test_plan_union.py): the source of an output element against a linear walk, a seam's position inside a chunk, rebased Utf8 offsets against
// offsets written out value by value, and the A-U6 limit checks at their edges.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "union.hpp"

using namespace flockgpu;

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            if (++fails < 10) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                            \
    } while (0)

static UnionSources table(const std::vector<uint32_t> &counts, uint32_t lo) {
    UnionSources S{};
    S.n = (int32_t)counts.size();
    uint32_t at = lo;
    for (int i = 0; i < S.n; ++i) {
        S.s[i].first = at;
        S.s[i].count = counts[(size_t)i];
        at += counts[(size_t)i];
    }
    S.lo = lo;
    S.hi = at;
    return S;
}

int main() {
    // the source of every element, and the seam inside every chunk of every width, against a linear walk over the table
    const std::vector<std::vector<uint32_t>> shapes = {{1}, {5}, {1, 1, 1}, {3, 5, 7, 1, 4097, 1}, {16, 16}, {15, 17, 1}, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}};
    for (auto &counts : shapes)
        for (uint32_t lo : {0u, 1u, 13u, 4096u}) {
            const UnionSources S = table(counts, lo);
            int k = 0;
            for (uint32_t e = S.lo; e < S.hi; ++e) {
                while (e >= S.s[k].first + S.s[k].count) ++k;
                CHECK(union_source_of(S, e) == k);
                for (uint32_t w : {2u, 4u, 16u}) {
                    uint32_t in = 0;   // elements e, e + 1, .. of source k among the next w
                    while (in < w && e + in < S.s[k].first + S.s[k].count) ++in;
                    CHECK(union_seam_in_chunk(S, k, e, w) == in);
                }
            }
            CHECK(k == S.n - 1);
        }
    {   // a table that ends at 2^31 - 1: no wrap in first + count
        const UnionSources S = table({(1u << 31) - 8, 7}, 0);
        CHECK(union_source_of(S, (1u << 31) - 9) == 0 && union_source_of(S, (1u << 31) - 8) == 1 && union_source_of(S, (1u << 31) - 2) == 1);
        CHECK(union_seam_in_chunk(S, 0, (1u << 31) - 10, 4) == 2 && union_seam_in_chunk(S, 1, (1u << 31) - 8, 16) == 7);
    }
    // rebased offsets against offsets written out value by value
    const std::vector<std::vector<uint32_t>> lens = {{0, 1, 15}, {}, {16, 17, 70, 0}, {1}};
    std::vector<uint64_t> want{0};
    uint64_t base = 0;
    size_t at = 0;
    for (auto &l : lens) {
        std::vector<uint64_t> off(l.size() + 1, 0);
        for (size_t i = 0; i < l.size(); ++i) off[i + 1] = off[i] + l[i];
        for (size_t i = 0; i < l.size(); ++i) {
            want.push_back(want.back() + l[i]);
            CHECK(union_rebased_offset(base, off[i]) == want[at]);
            ++at;
        }
        base += off.back();
    }
    CHECK(union_rebased_offset(base, 0) == want.back() && base == 120);
    CHECK(union_rebased_offset((1ull << 31) - 1, (1ull << 31) - 1) == (1ull << 32) - 2);
    // A-U6
    int64_t n = -1;
    const int64_t just[] = {(1ll << 31) - 2, 1, 0}, over[] = {(1ll << 31) - 2, 1, 1}, huge[] = {INT64_MAX, INT64_MAX, INT64_MAX}, one[] = {1ll << 31}, neg[] = {-5, 3};
    CHECK(union_rows_ok(just, 3, &n) && n == (1ll << 31) - 1);
    CHECK(!union_rows_ok(over, 3, &n) && n == 0);
    CHECK(!union_rows_ok(huge, 3, &n) && n == 0 && !union_rows_ok(one, 1, &n) && !union_bytes_ok(one, 1, &n) && !union_bytes_ok(over, 3, &n));
    CHECK(union_bytes_ok(just, 3, &n) && n == (1ll << 31) - 1);
    CHECK(union_rows_ok(neg, 2, &n) && n == 3 && union_rows_ok(neg, 0, &n) && n == 0);
    std::vector<int64_t> many(64, (1ll << 25));   // 64 inputs of 2^25 rows: 2^31 exactly
    CHECK(!union_rows_ok(many.data(), 64, &n));
    many[63] -= 1;
    CHECK(union_rows_ok(many.data(), 64, &n) && n == (1ll << 31) - 1);
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("union_index_test ok\n");
    return 0;
}
