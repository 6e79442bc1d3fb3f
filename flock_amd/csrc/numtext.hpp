// CAST(x AS Utf8) of an integer or a Timestamp(ms) (numtext.hip): the one way SQL makes text out of a number.  This header is the FORMATTING, plain C++
// that compiles on the host and on the device (tests/cpp/numtext_test.cpp checks it against snprintf and a day-by-day calendar): a value becomes a
// handful of 32-bit words that hold its bytes in memory order (byte i of the text at bits 8 * (i & 3) of word i >> 2), so that the emit kernel moves
// whole dwords and never a digit at a time.
//   digits10_u32 / _u64   the digit count from the leading-zero count and ONE table compare (bits * 1233 >> 12 approximates log10; the table says
//                         whether the value has reached the next power of ten) -- no loop over digits;
//   pair / quad           two (four) decimal digits as two (four) ASCII bytes; every division is by a constant: the 32-bit ones through the
//                         multiply-high of divmagic.hpp (one v_mul_hi_u32), the two 64-bit ones a value of more than eight digits needs are divisions
//                         by a compile-time constant, which the compiler lowers to its multiply-high;
//   integers              the value ZERO-PADDED to the full width of its type (12 / 20 digits: 3 / 5 words) -- eight digits per 32-bit remainder --, a
//                         '-' dropped over the padding in front of the first digit: the text is the LAST `len` bytes of the words (NumText::first = where);
//   timestamps            'YYYY-MM-DD HH:MM:SS[.mmm]' from calendar.hpp's split of the millisecond count into (day, millisecond of day) and of the day
//                         into a civil date: six words from byte 0 on, 19 bytes or -- a millisecond part that is not zero -- 23.
//
// Dialect and semantics (arrow-rs ~6 cast kernels: `lexical` for the integers, chrono's NaiveDateTime Display for timestamps; their source is not under
// the reference, so -- like textsel.hpp's A-T and textslice.hpp's A-SL lists -- ASSUMPTIONS, checked against tests/cast_text_ref.py and, there,
// against pyarrow.compute.cast):
//   A-NT1 cast_expr / try_cast_expr with cast_type Utf8 over an Int32, Int64, UInt64 or Timestamp(Millisecond) operand: a column, or any numeric
//         expression the general evaluator (valprog.hpp) takes -- CAST(price * 2 AS Utf8) --, which is evaluated into a temporary column first;
//   A-NT2 integers: the shortest decimal form, '-' for negatives, no '+', no padding; 0 is "0"; Int64's minimum is "-9223372036854775808" (20 bytes),
//         UInt64's maximum "18446744073709551615" (20 bytes);
//   A-NT3 Timestamp(ms): 'YYYY-MM-DD HH:MM:SS', followed by '.mmm' only when the millisecond part is not zero (19 or 23 bytes); the proleptic Gregorian
//         calendar, UTC; times before 1970 round towards minus infinity (-1 is '1969-12-31 23:59:59.999');
//   A-NT4 the years 0000 to 9999 are formatted: kNumTextTsMin .. kNumTextTsMax.  A row outside fails the execute by name under cast_expr (the way a zero
//         divisor fails a call, valprog.hpp A-V3) and gives NULL under try_cast_expr -- which otherwise equals cast_expr;
//   A-NT5 NULL in gives NULL out; the result is nullable;
//   A-NT6 refused by name at create / explain: a Float64 operand (Rust's shortest round-trip form has no counterpart here), a Boolean operand, a
//         numeric literal operand;
//   A-NT7 the result is an ordinary Utf8 column: wherever a text-valued expression is taken (textsel.hpp A-T1 / A-T4) the cast counts as a Utf8 COLUMN
//         -- a projected column, a branch of a text CASE (one of the sixteen sources, identical casts once), the value argument of a slice function
//         (textslice.hpp A-SL1), a GROUP BY / ORDER BY / DISTINCT key, the argument of COUNT / COUNT(DISTINCT).  Its bytes do not depend on batching
//         or grid shape;
//   Kept as before: text inside a condition or under an operator (CAST(i AS Utf8) = '5'), LIKE / char_length / octet_length over a cast.  (The way
//   back, a cast from Utf8 to a number or a timestamp, is textnum.hpp.)
#pragma once
#include <cstdint>

#include "calendar.hpp"
#include "divmagic.hpp"

namespace flockgpu {

constexpr int64_t kNumTextTsMin = -62167219200000;    // 0000-01-01 00:00:00
constexpr int64_t kNumTextTsMax = 253402300799999;    // 9999-12-31 23:59:59.999
constexpr int kNumTextMaxBytes = 23;

// What is formatted: the storage type, and Int64 storage read as Timestamp(ms)
enum class NumTextKind : int32_t { I32 = 0, I64 = 1, U64 = 2, TS = 3 };
constexpr int numtext_words(NumTextKind k) { return k == NumTextKind::I32 ? 3 : k == NumTextKind::TS ? 6 : 5; }
// the longest text of a kind: "-2147483648", "-9223372036854775808" / "18446744073709551615", 'YYYY-MM-DD HH:MM:SS.mmm'
constexpr int numtext_max_len(NumTextKind k) { return k == NumTextKind::I32 ? 11 : k == NumTextKind::TS ? 23 : 20; }

// A value's text: bytes [first, first + len) of the words
template <int kWords>
struct NumText {
    uint32_t w[kWords];
    uint32_t first, len;
};

namespace numtext {

constexpr UMod32 kBy10 = umod32_make(10), kBy100 = umod32_make(100), kBy10000 = umod32_make(10000), kBy1e8 = umod32_make(100000000);

FG_HD uint32_t clz32(uint32_t v) { return (uint32_t)__builtin_clz(v); }     // v > 0
FG_HD uint32_t clz64(uint64_t v) { return (uint32_t)__builtin_clzll(v); }   // v > 0

// decimal digits of v (0 has one): t = floor(bits * log10(2)) is the digit count or one short of it; v >= 10^t decides
FG_HD uint32_t digits10_u32(uint32_t v) {
    constexpr uint32_t p10[10] = {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u, 1000000000u};
    const uint32_t bits = 32u - clz32(v | 1u), t = (bits * 1233u) >> 12;   // t <= 9
    return t + ((v | 1u) >= p10[t] ? 1u : 0u);   // (v | 1: zero has one digit)
}
FG_HD uint32_t digits10_u64(uint64_t v) {
    constexpr uint64_t p10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull, 10000000000ull,
                                  100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull, 1000000000000000ull, 10000000000000000ull,
                                  100000000000000000ull, 1000000000000000000ull, 10000000000000000000ull};
    const uint32_t bits = 64u - clz64(v | 1ull), t = (bits * 1233u) >> 12;   // t <= 19
    return t + ((v | 1ull) >= p10[t] ? 1u : 0u);
}

// p < 100 as two ASCII bytes, the tens in the low byte
FG_HD uint32_t pair(uint32_t p) {
    const uint32_t tens = udiv32_apply(p, kBy10);
    return 0x3030u + tens + ((p - tens * 10u) << 8);
}
// v < 10000 as four ASCII bytes in memory order
FG_HD uint32_t quad(uint32_t v) {
    const uint32_t hi = udiv32_apply(v, kBy100);
    return pair(hi) | (pair(v - hi * 100u) << 16);
}
// v < 10^8 as eight ASCII bytes: *a the first four, *b the last
FG_HD void eight(uint32_t v, uint32_t *a, uint32_t *b) {
    const uint32_t hi = udiv32_apply(v, kBy10000);
    *a = quad(hi);
    *b = quad(v - hi * 10000u);
}

// word k of the words with a '-' at byte `at` of them
FG_HD uint32_t with_minus(uint32_t word, uint32_t k, uint32_t at) {
    const uint32_t sh = 8u * (at & 3u);
    return k == (at >> 2) ? (word & ~(0xffu << sh)) | ((uint32_t)'-' << sh) : word;
}

}  // namespace numtext

// |v| of a 32-bit value as twelve zero-padded digits, '-' in front of the first digit of a negative one
FG_HD NumText<3> numtext_u32(uint32_t mag, bool negative) {
    NumText<3> t;
    const uint32_t top = udiv32_apply(mag, numtext::kBy1e8);   // <= 42
    t.w[0] = numtext::quad(top);
    numtext::eight(mag - top * 100000000u, &t.w[1], &t.w[2]);
    t.len = numtext::digits10_u32(mag) + (negative ? 1u : 0u);
    t.first = 12u - t.len;
    if (negative) {
        t.w[0] = numtext::with_minus(t.w[0], 0, t.first);
        t.w[1] = numtext::with_minus(t.w[1], 1, t.first);
        t.w[2] = numtext::with_minus(t.w[2], 2, t.first);
    }
    return t;
}
FG_HD NumText<3> numtext_i32(int32_t v) { return numtext_u32(v < 0 ? 0u - (uint32_t)v : (uint32_t)v, v < 0); }

// ... of a 64-bit value as twenty
FG_HD NumText<5> numtext_u64(uint64_t mag, bool negative) {
    NumText<5> t;
    uint32_t low, mid = 0, top = 0;
    if (mag >> 32) {
        const uint64_t q = mag / 100000000ull;   // < 2^38
        low = (uint32_t)(mag - q * 100000000ull);
        if (q >> 32) {
            const uint64_t q2 = q / 100000000ull;   // <= 1844
            top = (uint32_t)q2;
            mid = (uint32_t)(q - q2 * 100000000ull);
        } else {
            top = udiv32_apply((uint32_t)q, numtext::kBy1e8);
            mid = (uint32_t)q - top * 100000000u;
        }
    } else {
        mid = udiv32_apply((uint32_t)mag, numtext::kBy1e8);
        low = (uint32_t)mag - mid * 100000000u;
    }
    t.w[0] = numtext::quad(top);
    numtext::eight(mid, &t.w[1], &t.w[2]);
    numtext::eight(low, &t.w[3], &t.w[4]);
    t.len = numtext::digits10_u64(mag) + (negative ? 1u : 0u);
    t.first = 20u - t.len;
    if (negative) {
        t.w[0] = numtext::with_minus(t.w[0], 0, t.first);
        t.w[1] = numtext::with_minus(t.w[1], 1, t.first);
        t.w[2] = numtext::with_minus(t.w[2], 2, t.first);
        t.w[3] = numtext::with_minus(t.w[3], 3, t.first);
        t.w[4] = numtext::with_minus(t.w[4], 4, t.first);
    }
    return t;
}
FG_HD NumText<5> numtext_i64(int64_t v) { return numtext_u64(v < 0 ? 0ull - (uint64_t)v : (uint64_t)v, v < 0); }

FG_HD bool numtext_ts_in_range(int64_t ms) { return ms >= kNumTextTsMin && ms <= kNumTextTsMax; }
// the length alone: 19, or 23 with a millisecond part (ms in range)
FG_HD uint32_t numtext_ts_len(int64_t ms) {
    const int64_t s = cal::floor_div<cal::kMsPerSecond>(ms);
    return ms - s * cal::kMsPerSecond != 0 ? 23u : 19u;
}
// 'YYYY-MM-DD HH:MM:SS[.mmm]' (ms in range)
FG_HD NumText<6> numtext_ts(int64_t ms) {
    NumText<6> t;
    const int64_t days = cal::floor_div<cal::kMsPerDay>(ms);
    const uint32_t in_day = (uint32_t)(ms - days * cal::kMsPerDay);   // [0, 86399999]
    const cal::Civil c = cal::civil_from_days(days);
    const uint32_t secs = in_day / 1000u, milli = in_day - secs * 1000u;
    const uint32_t mins = secs / 60u, sec = secs - mins * 60u;
    const uint32_t hour = mins / 60u, min = mins - hour * 60u;
    const uint32_t hh = numtext::pair(hour), hundreds = udiv32_apply(milli, numtext::kBy100);
    t.w[0] = numtext::quad((uint32_t)c.year);
    t.w[1] = (uint32_t)'-' | (numtext::pair((uint32_t)c.month) << 8) | ((uint32_t)'-' << 24);
    t.w[2] = numtext::pair((uint32_t)c.day) | ((uint32_t)' ' << 16) | ((hh & 0xffu) << 24);
    t.w[3] = (hh >> 8) | ((uint32_t)':' << 8) | (numtext::pair(min) << 16);
    t.w[4] = (uint32_t)':' | (numtext::pair(sec) << 8) | ((uint32_t)'.' << 24);
    t.w[5] = (0x30u + hundreds) | (numtext::pair(milli - hundreds * 100u) << 8);
    t.first = 0;
    t.len = milli ? 23u : 19u;
    return t;
}

#if defined(__HIPCC__)
// (device; numtext.hip, textenc.hip) The text `t` into the LDS stage at byte p.  x = the words between two zero words; byte d of x is the one that lands on the dword boundary at or below p:
// x moves down d >> 2 words (selects, one round per bit of the count: kMaxShift bounds it) and d & 3 bytes (a funnel shift of neighbouring words), and
// the aligned dwords that result are stored whole where all four bytes are the value's, byte by byte at its two ends.
template <int kWords, int kMaxShift>
__device__ __forceinline__ void numtext_place(uint8_t *stage, uint32_t p, const NumText<kWords> &t) {
    constexpr int kX = kWords + 2;
    uint32_t x[kX];
    x[0] = 0;
#pragma unroll
    for (int k = 0; k < kWords; ++k) x[k + 1] = t.w[k];
    x[kWords + 1] = 0;
    const uint32_t lo = p & 3u, hi = lo + t.len;   // bytes [lo, hi) of the aligned dwords are the value's
    const uint32_t d = t.first + 4u - lo;          // 1 .. 4 kWords + 3
    const uint32_t wi = d >> 2, sh = 8u * (d & 3u);
#pragma unroll
    for (int bit = 1; bit <= kMaxShift; bit <<= 1) {
        const bool on = (wi & (uint32_t)bit) != 0;
#pragma unroll
        for (int k = 0; k < kX; ++k) x[k] = on ? (k + bit < kX ? x[k + bit] : 0u) : x[k];
    }
    uint8_t *q = stage + (p - lo);
#pragma unroll
    for (int k = 0; k <= kWords; ++k) {
        const uint32_t b0 = 4u * (uint32_t)k;
        if (b0 >= hi) continue;
        const uint32_t a = __funnelshift_r(x[k], x[k + 1], sh);
        if (b0 >= lo && b0 + 4u <= hi) {
            *reinterpret_cast<uint32_t *>(q + b0) = a;
        } else {
#pragma unroll
            for (uint32_t c = 0; c < 4u; ++c)
                if (b0 + c >= lo && b0 + c < hi) q[b0 + c] = (uint8_t)(a >> (8u * c));
        }
    }
}
#endif

// byte i of the words (host tests, the emit kernel's tile edges)
template <int kWords>
FG_HD uint8_t numtext_byte(const NumText<kWords> &t, uint32_t i) {
    const uint32_t at = t.first + i;
    uint32_t v = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < kWords; ++k)
        if ((uint32_t)k == (at >> 2)) v = t.w[k];
    return (uint8_t)(v >> (8u * (at & 3u)));
}

}  // namespace flockgpu
