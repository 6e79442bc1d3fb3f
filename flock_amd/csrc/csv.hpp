// Delimited text (CSV, TPC-H '.tbl') -> columns (csv.hip): what ONE lane does with ONE record, as plain C++ that compiles on the host and on the
// device (tests/cpp/csv_test.cpp runs it under ASan / UBSan against a table of records, strtod and the timestamp edge cases):
//   csv_next_field   the walk over one field of a record's byte range, the quote rules included;
//   csv_f64          decimal text to Float64 where ONE IEEE operation gives the correctly rounded result, refused everywhere else;
//   csv_ts           textnum.hpp's Timestamp(ms) with up to nine fraction digits;
//   csv_value        one value of a column type from a field's bytes (the integers through textnum.hpp).
// A record's byte range comes from the record index of csv.hip (quote parity over 16 KiB tiles); the walk is bounded by that range and reads no byte
// outside it.
//
// Dialect and semantics.  The reference reads CSV with arrow's csv::ReaderBuilder (flock-function/src/aws/actor.rs:575-629: has_header(true),
// with_delimiter(b','), a given schema) and CsvReadOptions (playground/src/distributed_plan/partition.rs:157-179: delimiter(b'|')); the fork's arrow
// csv reader is not under the reference, so -- like textnum.hpp's A-TN list -- ASSUMPTIONS, checked against tests/csv_ref.py and, there, against
// Python's csv.reader(strict=True) and pyarrow.csv.read_csv:
//   A-CSV1 records: a record ends at '\n' or '\r\n' OUTSIDE quotes; a missing final terminator is fine.  has_header drops the first record unread
//          (its names are not compared with anything, as arrow does under a given schema).  A blank line (no byte between two terminators) is
//          refused with FLOCKGPU_ERR_UNSUPPORTED, as the JSON decoder refuses one; so is a bare '\r' outside quotes that no '\n' follows;
//   A-CSV2 fields are split at `delimiter`, any ASCII byte except '"', '\r' and '\n'.  A field that BEGINS with '"' is quoted: it runs to the closing
//          quote, '""' inside stands for one '"', delimiters, '\r' and '\n' inside are data.  A '"' anywhere else in an unquoted field, a byte between
//          a closing quote and the next delimiter or terminator, and a quote still open where the text ends fail with FLOCKGPU_ERR_INVALID;
//   A-CSV3 a record holds exactly n_fields fields, more or fewer fail with FLOCKGPU_ERR_INVALID.  A '.tbl' line ends in a trailing '|': that is one
//          more, empty, field, and its caller declares one more column of type SKIP for it;
//   A-CSV4 Int32 / Int64 / UInt64 are textnum.hpp A-TN1 exactly (textnum_int); Timestamp(ms) is A-TN2 with ONE difference, for this decoder only: the
//          fraction may have 1 to 9 digits, and digits after the third are dropped ('2020-11-01 00:11:32.6250' is ...32.625; the CAST does not
//          change).  A value of these types that does not parse fails with FLOCKGPU_ERR_INVALID.  The value is the field's bytes between the
//          quotes as they are: a quoted number that holds '""' does not parse;
//   A-CSV5 Float64 takes [+-]?digits[.digits][(e|E)[+-]?digits] and is converted only where the decimal significand without its trailing zeros is at
//          most 2^53 and the decimal exponent after folding the point (and those zeros) is in [-22, 22]: then double(w) and 10^|e| are both exact
//          and double(w) * 10^e or double(w) / 10^-e is ONE correctly rounded IEEE operation.  A zero significand is +-0 whatever the exponent.
//          Everything else -- more digits, larger exponents, 'inf', 'nan', hex, '1.', '.5' -- is refused with FLOCKGPU_ERR_UNSUPPORTED: no
//          almost-right double leaves the device (textnum.hpp A-TN5, narrowed rather than lifted);
//   A-CSV6 NULLs: an empty field, quoted or not, is NULL for every numeric type (validity 0, value 0); for Utf8 it is '', never NULL.  Utf8 bytes are
//          copied verbatim after unquoting; nothing checks that they are UTF-8;
//   A-CSV7 errors name the first offending record, 1-based with the header counted, and for a value the column and its type.  Inside a record the
//          first failure from the left decides.  On malformed quoting the record number is the one the quote-parity index yields: a stray quote
//          flips the parity, so the record it is reported for runs on to the next terminator that follows an even number of quotes.
#pragma once
#include <cstdint>

#include "textnum.hpp"

namespace flockgpu {

// (the values of include/flockgpu.h's FLOCKGPU_CSV_*)
enum : int32_t { kCsvSkip = -1, kCsvInt32 = 0, kCsvInt64 = 1, kCsvUInt64 = 2, kCsvFloat64 = 3, kCsvTimestampMs = 4, kCsvUtf8 = 5 };
enum : uint32_t {
    kCsvOk = 0, kCsvErrBlank = 1, kCsvErrBareCr = 2, kCsvErrStrayQuote = 3, kCsvErrAfterQuote = 4, kCsvErrOpenQuote = 5, kCsvErrFewFields = 6,
    kCsvErrManyFields = 7, kCsvErrValue = 8, kCsvErrFloat = 9
};

struct CsvField {
    int32_t begin, end;   // the value's raw bytes (between the quotes of a quoted field)
    int32_t ulen;         // its length after unquoting
    int32_t next;         // where the field ends: the delimiter's position, or the record's end
    bool dq;              // the value holds '""'
};

// One field of the record s[.. e): p is the field's first byte (p <= e; p == e is the empty last field).  0, or the kCsvErr* of the first rule
// that the field breaks
FG_HD uint32_t csv_next_field(const uint8_t *s, int32_t p, int32_t e, uint32_t delim, CsvField *f) {
    if (p < e && s[p] == (uint8_t)'"') {
        int32_t i = p + 1, ulen = 0;
        bool dq = false;
        for (;;) {
            if (i >= e) return kCsvErrOpenQuote;
            if (s[i] == (uint8_t)'"') {
                if (!(i + 1 < e && s[i + 1] == (uint8_t)'"')) break;   // the closing quote
                dq = true;
                ++i;
            }
            ++ulen;
            ++i;
        }
        f->begin = p + 1;
        f->end = i;
        f->ulen = ulen;
        f->dq = dq;
        f->next = i + 1;
        return i + 1 < e && s[i + 1] != delim ? kCsvErrAfterQuote : kCsvOk;
    }
    int32_t i = p;
    for (; i < e; ++i) {
        const uint32_t c = s[i];
        if (c == delim) break;
        if (c == (uint32_t)'"') return kCsvErrStrayQuote;
        if (c == (uint32_t)'\r') return kCsvErrBareCr;
    }
    f->begin = p;
    f->end = i;
    f->ulen = i - p;
    f->dq = false;
    f->next = i;
    return kCsvOk;
}

// The unquoting copy of a value that holds '""': s[b .. e) -> dst, the bytes written
FG_HD int32_t csv_unquote(const uint8_t *s, int32_t b, int32_t e, uint8_t *dst) {
    int32_t o = 0;
    for (int32_t i = b; i < e; ++i) {
        dst[o++] = s[i];
        if (s[i] == (uint8_t)'"') ++i;   // ('""': the walk has seen that the second one is there)
    }
    return o;
}

constexpr uint64_t kCsvMaxSignificand = uint64_t(1) << 53;
constexpr int kCsvMaxPow10 = 22;   // 10^22 = 2^22 * 5^22, and 5^22 < 2^53: the largest power of ten that is a double

// A-CSV5.  true: *out is THE double nearest to the text's value
FG_HD bool csv_f64(const uint8_t *p, int32_t len, double *out) {
    const double p10[kCsvMaxPow10 + 1] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    int32_t i = 0;
    bool negative = false;
    if (i < len && (p[i] == (uint8_t)'-' || p[i] == (uint8_t)'+')) negative = p[i++] == (uint8_t)'-';
    uint64_t w = 0;        // the significand's digits so far, without the `held` zeros at their end
    int64_t held = 0;      // zeros seen since the last non-zero digit (none while w is 0: zeros in front carry nothing)
    int64_t frac = 0;      // digits behind the point
    bool fits = true;
    for (int part = 0; part < 2; ++part) {
        const int32_t first = i;
        for (; i < len && p[i] >= (uint8_t)'0' && p[i] <= (uint8_t)'9'; ++i) {
            frac += part;
            const uint32_t d = (uint32_t)p[i] - (uint32_t)'0';
            if (d == 0u) {
                held += w != 0 ? 1 : 0;
                continue;
            }
            for (; held > 0 && fits; --held) {
                w *= 10u;   // (w <= 2^53 before: no wrap)
                fits = w <= kCsvMaxSignificand;
            }
            w = w * 10u + d;
            fits = fits && w <= kCsvMaxSignificand;
            if (!fits) return false;
        }
        if (i == first) return false;   // no digit where the form asks for one
        if (part == 1 || i >= len || p[i] != (uint8_t)'.') break;
        ++i;
    }
    int64_t exp10 = 0;
    if (i < len && (p[i] == (uint8_t)'e' || p[i] == (uint8_t)'E')) {
        ++i;
        bool eneg = false;
        if (i < len && (p[i] == (uint8_t)'-' || p[i] == (uint8_t)'+')) eneg = p[i++] == (uint8_t)'-';
        const int32_t first = i;
        for (; i < len && p[i] >= (uint8_t)'0' && p[i] <= (uint8_t)'9'; ++i) exp10 = exp10 < 1000000 ? exp10 * 10 + (int64_t)(p[i] - (uint8_t)'0') : exp10;
        if (i == first) return false;
        exp10 = eneg ? -exp10 : exp10;
    }
    if (i != len) return false;
    double v = 0.0;
    if (w != 0) {
        const int64_t e = exp10 - frac + held;
        if (e < -kCsvMaxPow10 || e > kCsvMaxPow10) return false;
        v = e < 0 ? (double)w / p10[-e] : (double)w * p10[e];
    }
    *out = negative ? -v : v;
    return true;
}

// A-CSV4: textnum.hpp's timestamp, and 'YYYY-MM-DD hh:mm:ss.' with four to nine fraction digits, of which the first three count
FG_HD bool csv_ts(const uint8_t *p, int32_t len, int64_t *out) {
    if (len > 23) {
        if (len > 29 || p[19] != (uint8_t)'.') return false;
        for (int32_t i = 23; i < len; ++i)
            if (p[i] < (uint8_t)'0' || p[i] > (uint8_t)'9') return false;
        len = 23;
    }
    return textnum_ts_bytes(p, len, out);
}

// One non-empty value of a numeric column type from its bytes: 0 and the value's bits (Int32 sign-extended), or kCsvErrValue / kCsvErrFloat
FG_HD uint32_t csv_value(int32_t type, const uint8_t *p, int32_t len, uint64_t *bits) {
    if (type == kCsvFloat64) {
        double v = 0.0;
        if (!csv_f64(p, len, &v)) return kCsvErrFloat;
        union { double d; uint64_t u; } x;
        x.d = v;
        *bits = x.u;
        return kCsvOk;
    }
    if (type == kCsvTimestampMs) {
        int64_t ms = 0;
        if (!csv_ts(p, len, &ms)) return kCsvErrValue;
        *bits = (uint64_t)ms;
        return kCsvOk;
    }
    const TextNumKind kind = type == kCsvInt32 ? TextNumKind::I32 : type == kCsvInt64 ? TextNumKind::I64 : TextNumKind::U64;
    return textnum_int_bytes(kind, p, len, bits) ? kCsvOk : kCsvErrValue;
}

}  // namespace flockgpu
