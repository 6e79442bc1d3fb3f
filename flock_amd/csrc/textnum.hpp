// CAST(x AS Int32 / Int64 / UInt64 / Timestamp(ms)) of a Utf8 value (textnum.hip): the way back from numtext.hpp.  This header is the PARSE of ONE value
// from bytes that are already in registers, plain C++ that compiles on the host and on the device (tests/cpp/textnum_test.cpp checks it against
// strtoll / strtoull, the edge table and the round trip through numtext.hpp).  A value arrives as a WINDOW of 24 bytes in three 64-bit words, byte i of
// the window at bits 8 * (i & 7) of word i >> 3 (memory order on a little-endian machine); what the window holds outside the value is never looked at.
//   integers     the window is RIGHT-aligned: it ends where the value ends, the value's first byte is byte 24 - len.  The sign byte and everything in
//                front of it are overwritten with '0' by a mask, so the window is always 24 digits: one range check per word (every byte in '0'..'9'),
//                the three-multiply reduction of eight ASCII digits to a number per word -- no byte loop.  Overflow: more than 20 significant digits is
//                a non-zero digit among the window's first four; twenty digits stay inside 64 bits when the first four are at most 1844 and the sum
//                does not carry; the rest is ONE compare of the magnitude against the type's limit;
//   timestamps   the window is LEFT-aligned.  The bytes behind the value are overwritten with the tail of '0000-00-00 00:00:00.000', so every form of
//                A-TN2 becomes the 23-byte one; XOR with that template turns digits into their values and separators into 0: one digit-class check
//                per word, one separator check, the fields picked by shifts; then a day-of-month table and calendar.hpp's days_from_civil;
//   a value of more than 24 bytes (leading zeros) goes through textnum_int_bytes, which steps over the zeros byte by byte and hands the rest to the
//   window parse: correct, not tuned.
//
// Dialect and semantics (arrow-rs ~6 cast kernels: `lexical` for the integers, string_to_timestamp_nanos for timestamps; their source is not under the
// reference, so -- like numtext.hpp's A-NT list -- ASSUMPTIONS, checked against tests/parse_text_ref.py and, there, against pyarrow.compute.cast):
//   A-TN1 integers: the WHOLE value is [+-]?[0-9]+.  Any number of leading zeros, any length.  No blanks, no '_', no exponent, no fraction, no
//         non-ASCII digits, NUL is not a digit; '', '-' and '+' do not parse.  The number must fit the target ('2147483648' is no Int32,
//         '-2147483648' is one).  '-0' is 0 for the signed types; for UInt64 any '-' does not parse, '-0' included.  A leading '+' IS accepted for
//         all three types (ASSUMPTION: Rust / lexical; pyarrow refuses it).  '0x10' does NOT parse (pyarrow reads it as hex: an Arrow C++ quirk that
//         is not adopted);
//   A-TN2 Timestamp(ms): 'YYYY-MM-DD', 'YYYY-MM-DD[ T]hh', '...hh:mm', '...hh:mm:ss', '...hh:mm:ss.f' / '.ff' / '.fff' -- the length decides the form.
//         Every field has exactly its digit count; the separator is 'T' (upper case) or one blank.  Month 1-12, the day valid for the month in the
//         proleptic Gregorian calendar ('1600-02-29' yes, '1900-02-29' no), hh 0-23, mm and ss 0-59: no leap second, no '24:00'.  No zone suffix;
//         the value is UTC.  Years 0000-9999, so that every text numtext.hpp prints parses back (ASSUMPTION: pyarrow refuses year 0000).
//         '1969-12-31 23:59:59.999' is -1.  More than three fraction digits do not parse;
//   A-TN3 under cast_expr a non-NULL value that does not parse fails the execute with FLOCKGPU_ERR_INVALID (the status of an unfit numeric CAST,
//         valprog.hpp A-V5), the message naming cast_expr, Utf8 and the target type; under try_cast_expr the row is NULL, and otherwise the two are
//         equal.  Every branch is evaluated for every row (A-V7): a failing row fails the call even under a CASE that would not pick it;
//   A-TN4 NULL in gives NULL out; the result is nullable; an all-NULL operand gives an all-NULL column and launches nothing;
//   A-TN5 refused by name at create / explain: cast_type Float64 (no correctly rounded decimal-to-double on the device, and an almost-right one would
//         break bit-exactness), Boolean, a Timestamp of another unit, a Utf8 literal operand;
//   A-TN6 the operand is a Utf8 column (read in place), a chain of slice functions over one (textslice.hpp: the parse reads the slice's per-row
//         (begin, end) pairs in place of the offsets, no byte is copied), or any other text-valued expression (a text CASE, a numtext.hpp cast, a slice
//         of those) through the materialisation those get as projected columns.  The result is an ordinary numeric column of the general evaluator
//         (valprog.hpp), as the text lengths are: usable under arithmetic, comparisons, CASE, IN, IS NULL, in predicates, and through
//         computed_column as a key, an aggregate argument and a join key.  Identical casts in one node are parsed once.
#pragma once
#include <cstdint>

#include "calendar.hpp"

namespace flockgpu {

enum class TextNumKind : int32_t { I32 = 0, I64 = 1, U64 = 2, TS = 3 };
constexpr int kTextNumWindow = 24;   // bytes of a window: a sign, twenty digits and three to spare; 'YYYY-MM-DD hh:mm:ss.fff' and one

struct TextNumWindow {
    uint64_t w[3];
};

namespace textnum {

constexpr uint64_t kZeros = 0x3030303030303030ull;

// the low n bytes of a word, n in [0, 8] after clamping
FG_HD uint64_t low_bytes(int n) { return n <= 0 ? 0ull : n >= 8 ? ~0ull : (1ull << (8 * n)) - 1ull; }
// every byte of v is in '0'..'9'
FG_HD bool all_digits(uint64_t v) {
    return ((v & 0xF0F0F0F0F0F0F0F0ull) | (((v + 0x0606060606060606ull) & 0xF0F0F0F0F0F0F0F0ull) >> 4)) == 0x3333333333333333ull;
}
// eight ASCII digits, the first in the low byte, as a number: pairs, quads, all eight -- three multiplies
FG_HD uint32_t eight_digits(uint64_t v) {
    v = ((v & 0x0F0F0F0F0F0F0F0Full) * 2561ull) >> 8;                 // 10 * 2^8 + 1
    v = ((v & 0x00FF00FF00FF00FFull) * 6553601ull) >> 16;             // 100 * 2^16 + 1
    return (uint32_t)(((v & 0x0000FFFF0000FFFFull) * 42949672960001ull) >> 32);   // 10000 * 2^32 + 1
}
// byte i of the window (i in [0, 24))
FG_HD uint32_t byte_at(const TextNumWindow &x, int i) {
    const uint64_t w = i < 8 ? x.w[0] : i < 16 ? x.w[1] : x.w[2];
    return (uint32_t)(w >> (8 * (i & 7))) & 0xffu;
}

// The digits of a right-aligned window whose first `fill` bytes are not part of the number: *out = the value's bits in the type of `kind`
FG_HD bool digits(TextNumKind kind, TextNumWindow x, int fill, bool negative, uint64_t *out) {
    if (fill >= kTextNumWindow) return false;   // no digit
    // the last eight bytes always; the eight in front of them and the first eight only where the value reaches them (a short number is one word's work)
    const uint64_t m2 = low_bytes(fill - 16);
    const uint64_t w2 = (x.w[2] & ~m2) | (kZeros & m2);
    bool ok = all_digits(w2);
    uint64_t lo = eight_digits(w2);
    uint32_t hi = 0;   // the first four of the twenty: <= 9999
    if (fill < 16) {
        const uint64_t m1 = low_bytes(fill - 8);
        const uint64_t w1 = (x.w[1] & ~m1) | (kZeros & m1);
        ok = ok && all_digits(w1);
        lo += (uint64_t)eight_digits(w1) * 100000000ull;
        if (fill < 8) {
            const uint64_t m0 = low_bytes(fill);
            const uint64_t w0 = (x.w[0] & ~m0) | (kZeros & m0);
            ok = ok && all_digits(w0) && !((uint32_t)w0 & 0x0F0F0F0Fu);   // (... and no more than twenty significant digits)
            hi = eight_digits(w0);
        }
    }
    if (!ok) return false;
    const uint64_t n = negative ? 1ull : 0ull;
    const uint64_t limit = kind == TextNumKind::I32 ? 2147483647ull + n : kind == TextNumKind::U64 ? ~0ull : 9223372036854775807ull + n;
    const uint64_t mag = (uint64_t)hi * 10000000000000000ull + lo;   // (1844 * 10^16 < 2^64)
    if (hi > 1844u || mag < lo || mag > limit) return false;
    *out = negative ? 0ull - mag : mag;
    return true;
}

constexpr uint64_t kTsT0 = 0x2D30302D30303030ull;   // '0000-00-'
constexpr uint64_t kTsT1 = 0x30303A3030203030ull;   // '00 00:00'
constexpr uint64_t kTsT2 = 0x003030302E30303Aull;   // ':00.000' and a zero byte
// every byte of v (bit 7 clear or not) is at most 9
FG_HD bool all_small(uint64_t v) { return ((((v & 0x7F7F7F7F7F7F7F7Full) + 0x7676767676767676ull) | v) & 0x8080808080808080ull) == 0; }
// the two digit values at bytes i and i + 1 of a word as a number
FG_HD uint32_t two(uint64_t v, int i) { return (uint32_t)((v >> (8 * i)) & 0xffu) * 10u + (uint32_t)((v >> (8 * i + 8)) & 0xffu); }

}  // namespace textnum

// An integer from a RIGHT-aligned window: the value is bytes [24 - len, 24).  len in [0, 24]
FG_HD bool textnum_int(TextNumKind kind, const TextNumWindow &x, int len, uint64_t *out) {
    if (len <= 0 || len > kTextNumWindow) return false;
    const int first = kTextNumWindow - len;
    const uint32_t c = textnum::byte_at(x, first);
    const bool negative = c == (uint32_t)'-', sign = negative || c == (uint32_t)'+';
    if (negative && kind == TextNumKind::U64) return false;
    return textnum::digits(kind, x, first + (sign ? 1 : 0), negative, out);
}

// A Timestamp(ms) from a LEFT-aligned window: the value is bytes [0, len)
FG_HD bool textnum_ts(TextNumWindow x, int len, int64_t *out) {
    using namespace textnum;
    if (len < 10 || len > 23 || !((1u << len) & ((1u << 10) | (1u << 13) | (1u << 16) | (1u << 19) | (1u << 21) | (1u << 22) | (1u << 23)))) return false;
    const uint64_t k1 = low_bytes(len - 8), k2 = low_bytes(len - 16);   // (len >= 10: word 0 is the value's)
    x.w[1] = (x.w[1] & k1) | (kTsT1 & ~k1);
    x.w[2] = (x.w[2] & k2) | (kTsT2 & ~k2);
    if (((x.w[1] >> 16) & 0xffu) == (uint64_t)'T') x.w[1] ^= (uint64_t)('T' ^ ' ') << 16;
    const uint64_t a = x.w[0] ^ kTsT0, b = x.w[1] ^ kTsT1, c = x.w[2] ^ kTsT2;   // digits: their values; separators: 0
    if (!all_small(a) || !all_small(b) || !all_small(c)) return false;
    if ((a & 0xFF0000FF00000000ull) | (b & 0x0000FF0000FF0000ull) | (c & 0xFF000000FF0000FFull)) return false;   // bytes 4, 7; 10, 13; 16, 19, 23
    const uint32_t year = two(a, 0) * 100u + two(a, 2), month = two(a, 5), day = two(b, 0), hh = two(b, 3), mm = two(b, 6), ss = two(c, 1);
    const uint32_t milli = (uint32_t)((c >> 32) & 0xffu) * 100u + two(c, 5);
    if (month < 1u || month > 12u || hh > 23u || mm > 59u || ss > 59u) return false;
    const bool leap = (year % 4u == 0u && year % 100u != 0u) || year % 400u == 0u;
    // days of the months January .. December, four bits each above 28
    const uint32_t dim = 28u + (uint32_t)((0x323233232303ull >> (4u * (month - 1u))) & 0xfu) + (month == 2u && leap ? 1u : 0u);
    if (day < 1u || day > dim) return false;
    const int64_t days = cal::days_from_civil((int64_t)year, (int32_t)month, (int32_t)day);
    *out = days * cal::kMsPerDay + (int64_t)(hh * 3600000u + mm * 60000u + ss * 1000u + milli);
    return true;
}

// A window from bytes in memory, one at a time (the host tests; the kernel's plain path): [p, p + len), len <= 24
FG_HD TextNumWindow textnum_window(const uint8_t *p, int len, bool right) {
    uint64_t w0 = 0, w1 = 0, w2 = 0;   // (three names, no indexed array: the words stay in registers on the device)
    const int at = right ? kTextNumWindow - len : 0;
    for (int i = 0; i < len; ++i) {
        const int pos = at + i;
        const uint64_t v = (uint64_t)p[i] << (8 * (pos & 7));
        w0 |= pos < 8 ? v : 0ull;
        w1 |= pos >= 8 && pos < 16 ? v : 0ull;
        w2 |= pos >= 16 ? v : 0ull;
    }
    TextNumWindow x;
    x.w[0] = w0;
    x.w[1] = w1;
    x.w[2] = w2;
    return x;
}

// A value of any length, byte by byte where it is longer than a window: the sign, the zeros in front, then the window parse of what is left
FG_HD bool textnum_int_bytes(TextNumKind kind, const uint8_t *p, int64_t len, uint64_t *out) {
    if (len <= kTextNumWindow) return textnum_int(kind, textnum_window(p, (int)len, true), (int)len, out);
    const bool negative = p[0] == (uint8_t)'-', sign = negative || p[0] == (uint8_t)'+';
    if (negative && kind == TextNumKind::U64) return false;
    int64_t i = sign ? 1 : 0;
    while (i < len - 1 && p[i] == (uint8_t)'0') ++i;
    if (len - i > 20) return false;   // more than twenty digits that do not begin with a zero, or something that is no digit
    const int rest = (int)(len - i);
    return textnum::digits(kind, textnum_window(p + i, rest, true), kTextNumWindow - rest, negative, out);   // (a second sign is no digit)
}
FG_HD bool textnum_ts_bytes(const uint8_t *p, int64_t len, int64_t *out) {
    if (len < 10 || len > 23) return false;
    return textnum_ts(textnum_window(p, (int)len, false), (int)len, out);
}

// one value of `kind`, whatever its length: the bits of the result (Int32 sign-extended)
FG_HD bool textnum_bytes(TextNumKind kind, const uint8_t *p, int64_t len, uint64_t *out) {
    if (kind != TextNumKind::TS) return textnum_int_bytes(kind, p, len, out);
    int64_t ms = 0;
    const bool ok = textnum_ts_bytes(p, len, &ms);
    *out = (uint64_t)ms;
    return ok;
}

}  // namespace flockgpu
