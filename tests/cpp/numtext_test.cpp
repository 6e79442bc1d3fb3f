// flock_amd/csrc/numtext.hpp on the CPU (g++, address and undefined-behaviour sanitizers): the text of an integer against snprintf -- every power of
// ten and of two plus and minus one for 32 and 64 bits, signed and unsigned, the extreme values, a few thousand pseudo-random ones --, and the text of a
// Timestamp(ms) against a calendar walked day by day with the Gregorian leap rule from 0000-01-01 to 9999-12-31: the first and the last millisecond of
// every day that is a year's first or last or the 97th since the last one checked, a moment inside it, the two edges of the range and one value beyond each.
// Prints "numtext_test: ok <checks>" and exits 0, or the first difference and exits 1.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>

#include "numtext.hpp"

using namespace flockgpu;

static long g_checks = 0;

template <int W>
static std::string text_of(const NumText<W> &t) {
    std::string s;
    for (uint32_t i = 0; i < t.len; ++i) s.push_back((char)numtext_byte(t, i));
    return s;
}

#define CHECK(cond, ...)              \
    do {                              \
        ++g_checks;                   \
        if (!(cond)) {                \
            std::printf(__VA_ARGS__); \
            std::printf("\n");        \
            return 1;                 \
        }                             \
    } while (0)

static int check_u64(uint64_t v) {
    char want[32];
    std::snprintf(want, sizeof want, "%" PRIu64, v);
    const NumText<5> t = numtext_u64(v, false);
    CHECK(t.first + t.len == 20 && text_of(t) == want, "u64 %s: got '%s' (len %u)", want, text_of(t).c_str(), t.len);
    CHECK(numtext::digits10_u64(v) == std::strlen(want), "digits10_u64(%s) = %u", want, numtext::digits10_u64(v));
    return 0;
}
static int check_i64(int64_t v) {
    char want[32];
    std::snprintf(want, sizeof want, "%" PRId64, v);
    const NumText<5> t = numtext_i64(v);
    CHECK(t.first + t.len == 20 && text_of(t) == want, "i64 %s: got '%s' (len %u)", want, text_of(t).c_str(), t.len);
    return 0;
}
static int check_u32(uint32_t v) {
    char want[32];
    std::snprintf(want, sizeof want, "%" PRIu32, v);
    const NumText<3> t = numtext_u32(v, false);
    CHECK(t.first + t.len == 12 && text_of(t) == want, "u32 %s: got '%s' (len %u)", want, text_of(t).c_str(), t.len);
    CHECK(numtext::digits10_u32(v) == std::strlen(want), "digits10_u32(%s) = %u", want, numtext::digits10_u32(v));
    return 0;
}
static int check_i32(int32_t v) {
    char want[32];
    std::snprintf(want, sizeof want, "%" PRId32, v);
    const NumText<3> t = numtext_i32(v);
    CHECK(t.first + t.len == 12 && text_of(t) == want, "i32 %s: got '%s' (len %u)", want, text_of(t).c_str(), t.len);
    return 0;
}
// every width a value is cast at
static int check_all(uint64_t v) {
    if (check_u64(v) || check_i64((int64_t)v) || check_u32((uint32_t)v) || check_i32((int32_t)(uint32_t)v)) return 1;
    if (check_i64(-(int64_t)(v & 0x7fffffffffffffffull)) || check_i32(-(int32_t)(v & 0x7fffffffu))) return 1;
    return 0;
}

static bool leap(int y) { return (y % 4 == 0 && y % 100 != 0) || y % 400 == 0; }
static int month_days(int y, int m) {
    static const int d[] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    return m == 2 && leap(y) ? 29 : d[m - 1];
}
static int check_ts(int64_t ms, int y, int mo, int d, int h, int mi, int s, int frac) {
    char want[40];
    if (frac) std::snprintf(want, sizeof want, "%04d-%02d-%02d %02d:%02d:%02d.%03d", y, mo, d, h, mi, s, frac);
    else std::snprintf(want, sizeof want, "%04d-%02d-%02d %02d:%02d:%02d", y, mo, d, h, mi, s);
    CHECK(numtext_ts_in_range(ms), "%s (%lld) is taken to be out of range", want, (long long)ms);
    const NumText<6> t = numtext_ts(ms);
    CHECK(t.first == 0 && text_of(t) == want, "ts %lld: got '%s', want '%s'", (long long)ms, text_of(t).c_str(), want);
    CHECK(numtext_ts_len(ms) == std::strlen(want), "numtext_ts_len(%lld) = %u", (long long)ms, numtext_ts_len(ms));
    return 0;
}

int main() {
    // integers
    uint64_t p10 = 1;
    for (int k = 0; k < 20; ++k, p10 *= 10) {
        if (check_all(p10) || check_all(p10 - 1) || check_all(p10 + 1)) return 1;
    }
    for (int k = 0; k < 64; ++k) {
        const uint64_t p2 = uint64_t(1) << k;
        if (check_all(p2) || check_all(p2 - 1) || check_all(p2 + 1)) return 1;
    }
    if (check_all(0) || check_u64(UINT64_MAX) || check_i64(INT64_MIN) || check_i64(INT64_MAX) || check_u32(UINT32_MAX) || check_i32(INT32_MIN) || check_i32(INT32_MAX)) return 1;
    if (check_u64(uint64_t(1) << 63) || check_u64(9999999999999999999ull) || check_u64(10000000000000000000ull)) return 1;
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (int k = 0; k < 4000; ++k) {   // xorshift values cut to every length
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        if (check_all(x >> (k % 64))) return 1;
    }
    for (uint32_t p = 0; p < 100; ++p) CHECK(numtext::pair(p) == (uint32_t)(0x3030 + p / 10 + ((p % 10) << 8)), "pair(%u)", p);
    for (uint32_t v = 0; v < 10000; ++v) {
        char want[8];
        std::snprintf(want, sizeof want, "%04u", v);
        const uint32_t q = numtext::quad(v);
        CHECK(std::memcmp(&q, want, 4) == 0, "quad(%u)", v);
    }
    // timestamps: the calendar from 0000-01-01 (a leap year in the proleptic calendar) on, day by day
    int64_t day = 0;
    for (int y = 1969; y >= 0; --y) day -= leap(y) ? 366 : 365;
    CHECK(day * cal::kMsPerDay == kNumTextTsMin, "0000-01-01 is day %lld", (long long)day);
    long since = 0;
    for (int y = 0; y <= 9999; ++y)
        for (int m = 1; m <= 12; ++m)
            for (int d = 1; d <= month_days(y, m); ++d, ++day, ++since) {
                const bool year_edge = (m == 1 && d == 1) || (m == 12 && d == 31), leap_day = m == 2 && d >= 28, near_epoch = y >= 1969 && y <= 1971;
                if (!year_edge && !leap_day && !near_epoch && since < 97) continue;
                since = 0;
                const int64_t ms0 = day * cal::kMsPerDay;
                if (check_ts(ms0, y, m, d, 0, 0, 0, 0) || check_ts(ms0 + cal::kMsPerDay - 1, y, m, d, 23, 59, 59, 999)) return 1;
                if (check_ts(ms0 + 1, y, m, d, 0, 0, 0, 1) || check_ts(ms0 + cal::kMsPerDay - 1000, y, m, d, 23, 59, 59, 0)) return 1;
                const int h = (int)(day % 24 + 24) % 24, mi = (int)(day % 60 + 60) % 60, s = (int)(day % 59 + 59) % 59;
                static const int fracs[] = {0, 1, 10, 100, 999, 120, 5};
                const int f = fracs[(day % 7 + 7) % 7];
                if (check_ts(ms0 + h * cal::kMsPerHour + mi * cal::kMsPerMinute + s * cal::kMsPerSecond + f, y, m, d, h, mi, s, f)) return 1;
            }
    CHECK(day * cal::kMsPerDay - 1 == kNumTextTsMax, "9999-12-31 ends at %lld", (long long)(day * cal::kMsPerDay - 1));
    if (check_ts(-1, 1969, 12, 31, 23, 59, 59, 999) || check_ts(0, 1970, 1, 1, 0, 0, 0, 0) || check_ts(1456704000000, 2016, 2, 29, 0, 0, 0, 0)) return 1;
    if (check_ts(kNumTextTsMin, 0, 1, 1, 0, 0, 0, 0) || check_ts(kNumTextTsMax, 9999, 12, 31, 23, 59, 59, 999)) return 1;
    CHECK(!numtext_ts_in_range(kNumTextTsMin - 1) && !numtext_ts_in_range(kNumTextTsMax + 1) && !numtext_ts_in_range(INT64_MIN) && !numtext_ts_in_range(INT64_MAX),
          "a value beyond the range is taken to be inside it");
    std::printf("numtext_test: ok %ld\n", g_checks);
    return 0;
}
