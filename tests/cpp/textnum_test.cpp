// flock_amd/csrc/textnum.hpp on the CPU (g++, optionally with the address and undefined-behaviour sanitizers): the parse of an integer against
// strtoll / strtoull plus the explicit rules of A-TN1 on an edge table, the parse of a Timestamp(ms) on the forms of A-TN2 and a malformed neighbour of
// each, and the round trip through numtext.hpp -- every power of ten plus and minus one, every type's limits plus and minus one, 10^6 pseudo-random
// values per type, and 00:00:00 and 23:59:59.999 of every day from 0000-01-01 to 9999-12-31.  Every value goes through the window parse (24 bytes in
// registers) and through textnum_bytes; values behind a run of zeros go through the long path.
// Prints "textnum_test: ok <checks>" and exits 0, or the first difference and exits 1.
#include <cerrno>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "numtext.hpp"
#include "textnum.hpp"

using namespace flockgpu;

static long g_checks = 0;

#define CHECK(cond, ...)              \
    do {                              \
        ++g_checks;                   \
        if (!(cond)) {                \
            std::printf(__VA_ARGS__); \
            std::printf("\n");        \
            return 1;                 \
        }                             \
    } while (0)

template <int W>
static std::string text_of(const NumText<W> &t) {
    std::string s;
    for (uint32_t i = 0; i < t.len; ++i) s.push_back((char)numtext_byte(t, i));
    return s;
}

// the bytes of `s` in a buffer of their own size (a read past them is a sanitizer finding)
static bool parse(TextNumKind k, const std::string &s, uint64_t *out) {
    std::vector<uint8_t> b(s.begin(), s.end());
    uint8_t none = 0;
    return textnum_bytes(k, b.empty() ? &none : b.data(), (int64_t)b.size(), out);
}

// A-TN1 by the book: [+-]?[0-9]+ and the range, through strtoull on the digits
static bool want_int(TextNumKind k, const std::string &s, uint64_t *out) {
    size_t i = 0;
    bool neg = false;
    if (i < s.size() && (s[i] == '+' || s[i] == '-')) neg = s[i++] == '-';
    if (i == s.size()) return false;
    for (size_t j = i; j < s.size(); ++j)
        if (s[j] < '0' || s[j] > '9') return false;
    if (neg && k == TextNumKind::U64) return false;
    errno = 0;
    const std::string digits = s.substr(i);   // (no embedded NUL: all digits)
    const unsigned long long mag = std::strtoull(digits.c_str(), nullptr, 10);
    if (errno == ERANGE) return false;
    const uint64_t lim = k == TextNumKind::I32 ? 2147483647ull + neg : k == TextNumKind::I64 ? 9223372036854775807ull + neg : UINT64_MAX;
    if (mag > lim) return false;
    *out = neg ? 0ull - (uint64_t)mag : (uint64_t)mag;
    return true;
}

static int check_int(const std::string &s) {
    for (TextNumKind k : {TextNumKind::I32, TextNumKind::I64, TextNumKind::U64}) {
        uint64_t got = 0, want = 0;
        const bool g = parse(k, s, &got), w = want_int(k, s, &want);
        CHECK(g == w && (!g || got == want), "kind %d '%s': got %d %" PRIu64 ", want %d %" PRIu64, (int)k, s.c_str(), (int)g, got, (int)w, want);
    }
    return 0;
}
// ... and with zeros in front, short and beyond a window
static int check_int_padded(const std::string &s) {
    if (check_int(s)) return 1;
    const bool sign = !s.empty() && (s[0] == '+' || s[0] == '-');
    for (int z : {1, 3, 4, 13, 24, 25, 70}) {
        const std::string t = (sign ? s.substr(0, 1) : std::string()) + std::string((size_t)z, '0') + s.substr(sign ? 1 : 0);
        if (check_int(t)) return 1;
    }
    return 0;
}

static int check_ts(const std::string &s, bool ok, int64_t want) {
    uint64_t got = 0;
    const bool g = parse(TextNumKind::TS, s, &got);
    CHECK(g == ok && (!g || (int64_t)got == want), "ts '%s': got %d %" PRId64 ", want %d %" PRId64, s.c_str(), (int)g, (int64_t)got, (int)ok, want);
    return 0;
}
static int round_trip_ts(int64_t ms) {
    const std::string s = text_of(numtext_ts(ms));
    if (check_ts(s, true, ms)) return 1;
    std::string t = s;
    t[10] = 'T';
    return check_ts(t, true, ms);
}
static int round_trip(uint64_t v) {
    uint64_t got = 0;
    const std::string u = text_of(numtext_u64(v, false)), i = text_of(numtext_i64((int64_t)v)), w = text_of(numtext_i32((int32_t)(uint32_t)v));
    CHECK(parse(TextNumKind::U64, u, &got) && got == v, "u64 round trip of %s", u.c_str());
    CHECK(parse(TextNumKind::I64, i, &got) && got == v, "i64 round trip of %s", i.c_str());
    CHECK(parse(TextNumKind::I32, w, &got) && (int64_t)got == (int64_t)(int32_t)(uint32_t)v, "i32 round trip of %s", w.c_str());
    return check_int_padded(u) || check_int_padded(i) || check_int_padded(w) || check_int_padded("+" + u);
}

int main() {
    // the edge table
    const char *edges[] = {"0", "-0", "+0", "+5", "-5", "007", "-007", "+007", " 5", "5 ", "", "-", "+", "--5", "+-5", "-+5", "5-", "5+", "1e3", "1.0", "5a", "a5", "0x10", "0X10", "1_000",
                           "2147483647", "2147483648", "-2147483648", "-2147483649", "9223372036854775807", "9223372036854775808", "-9223372036854775808",
                           "-9223372036854775809", "18446744073709551615", "18446744073709551616", "18446744073709551614", "-18446744073709551615",
                           "99999999999999999999", "100000000000000000000", "28446744073709551615", "18446744073709551615000", "\xd9\xa5", "\xef\xbc\x95", "5\xd9\xa5", "/", ":", "5/", "5:"};
    for (const char *e : edges)
        if (check_int_padded(e)) return 1;
    if (check_int(std::string("5\0", 2)) || check_int(std::string("\0" "5", 2)) || check_int(std::string("1\0" "2", 3)) || check_int(std::string(1, '\0'))) return 1;
    if (check_int(std::string(40000, '0') + "7") || check_int("-" + std::string(40000, '0') + "7") || check_int(std::string(40000, '0') + "-7") ||
        check_int("+" + std::string(30, '0') + "+7") || check_int(std::string(30, '0')) || check_int(std::string(30, '1')) || check_int(std::string(25, '0') + " "))
        return 1;
    // integers: the round trip through numtext.hpp
    uint64_t p10 = 1;
    for (int k = 0; k < 20; ++k, p10 *= 10)
        if (round_trip(p10) || round_trip(p10 - 1) || round_trip(p10 + 1) || round_trip(0 - p10) || round_trip(0 - p10 + 1) || round_trip(0 - p10 - 1)) return 1;
    for (uint64_t lim : {(uint64_t)INT32_MAX, (uint64_t)(int64_t)INT32_MIN, (uint64_t)INT64_MAX, (uint64_t)INT64_MIN, UINT64_MAX, (uint64_t)0, (uint64_t)UINT32_MAX})
        if (round_trip(lim) || round_trip(lim - 1) || round_trip(lim + 1)) return 1;
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (int k = 0; k < 1000000; ++k) {   // xorshift values cut to every length
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const uint64_t v = x >> (k % 64);
        uint64_t got = 0;
        const std::string u = text_of(numtext_u64(v, false)), i = text_of(numtext_i64((int64_t)(v * 3))), w = text_of(numtext_i32((int32_t)(uint32_t)(v * 3)));
        CHECK(parse(TextNumKind::U64, u, &got) && got == v, "u64 round trip of %s", u.c_str());
        CHECK(parse(TextNumKind::I64, i, &got) && got == v * 3, "i64 round trip of %s", i.c_str());
        CHECK(parse(TextNumKind::I32, w, &got) && (int64_t)got == (int64_t)(int32_t)(uint32_t)(v * 3), "i32 round trip of %s", w.c_str());
        if (k % 1000 == 0 && (check_int(u) || check_int(i) || check_int(w))) return 1;
    }
    for (uint32_t v = 0; v < 100000; ++v) {   // the three-multiply reduction on its own
        char t[16];
        std::snprintf(t, sizeof t, "%08u", v * 999u);
        uint64_t word;
        std::memcpy(&word, t, 8);
        CHECK(textnum::all_digits(word) && textnum::eight_digits(word) == v * 999u, "eight_digits('%s')", t);
    }
    // timestamps: every form and a malformed neighbour of each
    const int64_t d0 = 1436918400000;   // 2015-07-15
    struct { const char *s; bool ok; int64_t ms; } ts[] = {
        {"2015-07-15", true, d0}, {"2015-07-1", false, 0}, {"2015-7-15", false, 0}, {"2015/07/15", false, 0}, {"2015-07-15 ", false, 0},
        {"2015-07-15 09", true, d0 + 9 * 3600000}, {"2015-07-15T09", true, d0 + 9 * 3600000}, {"2015-07-15t09", false, 0}, {"2015-07-15 9", false, 0}, {"2015-07-15  9", false, 0},
        {"2015-07-15 09:08", true, d0 + 9 * 3600000 + 8 * 60000}, {"2015-07-15 09-08", false, 0}, {"2015-07-15 09:8", false, 0}, {"2015-07-15 09:", false, 0},
        {"2015-07-15 09:08:07", true, d0 + 9 * 3600000 + 8 * 60000 + 7000}, {"2015-07-15 09:08.07", false, 0}, {"2015-07-15 09:08:7", false, 0}, {"2015-07-15 09:08:", false, 0},
        {"2015-07-15 09:08:07.1", true, d0 + 9 * 3600000 + 8 * 60000 + 7100}, {"2015-07-15 09:08:07.", false, 0}, {"2015-07-15 09:08:07,1", false, 0},
        {"2015-07-15 09:08:07.12", true, d0 + 9 * 3600000 + 8 * 60000 + 7120}, {"2015-07-15 09:08:07.1a", false, 0},
        {"2015-07-15 09:08:07.123", true, d0 + 9 * 3600000 + 8 * 60000 + 7123}, {"2015-07-15 09:08:07.12 ", false, 0}, {"2015-07-15 09:08:07.1234", false, 0},
        {"2015-07-15T09:08:07.123", true, d0 + 9 * 3600000 + 8 * 60000 + 7123}, {"2015-07-15 09:08:07Z", false, 0}, {"2015-07-15 09:08:07+00", false, 0},
        {"1900-02-29", false, 0}, {"1600-02-29", true, -11670998400000}, {"2015-02-29", false, 0}, {"2016-02-29", true, 1456704000000}, {"2015-04-31", false, 0}, {"2015-00-10", false, 0},
        {"2015-13-10", false, 0}, {"2015-01-00", false, 0}, {"2015-01-32", false, 0}, {"0000-01-01 00:00:00", true, kNumTextTsMin}, {"9999-12-31 23:59:59.999", true, kNumTextTsMax},
        {"2015-07-15 24:00", false, 0}, {"2015-07-15 23:60", false, 0}, {"2015-07-15 23:59:60", false, 0}, {"2015-07-15 00:00:00.1234", false, 0},
        {"1969-12-31 23:59:59.999", true, -1}, {"1970-01-01", true, 0}, {"", false, 0}, {"2015", false, 0}, {"-2015-07-15", false, 0}, {"+015-07-15", false, 0},
        {"2015-07-15 09:08:07.\xd9\xa5", false, 0}, {"20\xd9\xa5-07-15", false, 0}, {" 2015-07-15", false, 0}, {"10000-01-01", false, 0}};
    for (auto &t : ts)
        if (check_ts(t.s, t.ok, t.ms)) return 1;
    if (check_ts(std::string("2015-07-15\0", 11), false, 0) || check_ts(std::string("2015-07-15 0\0", 13), false, 0)) return 1;
    // every day of the years 0000 to 9999
    for (int64_t day = kNumTextTsMin / cal::kMsPerDay; day * cal::kMsPerDay <= kNumTextTsMax; ++day) {
        if (round_trip_ts(day * cal::kMsPerDay) || round_trip_ts(day * cal::kMsPerDay + cal::kMsPerDay - 1)) return 1;
        if (day % 97 == 0) {
            const int64_t ms = day * cal::kMsPerDay + (((day % 24) + 24) % 24) * cal::kMsPerHour + (((day % 60) + 60) % 60) * cal::kMsPerMinute + (((day % 59) + 59) % 59) * 1000 + (((day % 7) + 7) % 7) * 110;
            if (round_trip_ts(ms)) return 1;
            const std::string s = text_of(numtext_ts(ms));
            for (size_t cut : {(size_t)10, (size_t)13, (size_t)16, (size_t)19}) {   // the shorter forms are the longer ones cut
                uint64_t a = 0, b = 0;
                std::string full = s.substr(0, cut) + std::string("0000-00-00 00:00:00").substr(cut);
                full[5] = s[5]; full[6] = s[6]; full[8] = s[8]; full[9] = s[9];
                CHECK(parse(TextNumKind::TS, s.substr(0, cut), &a) && parse(TextNumKind::TS, full, &b) && a == b, "the form of %zu bytes of '%s'", cut, s.c_str());
            }
        }
    }
    std::printf("textnum_test: ok %ld\n", g_checks);
    return 0;
}
