// Columns -> text (textenc.hip): flockgpu_json_lines_encode and flockgpu_csv_encode, the way back from json.hip and csv.hip.  This header is the RULES
// as plain C++ that compiles on the host and on the device (tests/cpp/textenc_test.cpp checks every function against a byte loop): which bytes of a Utf8
// value make it grow (the byte classes, per byte and per little-endian dword), what one byte becomes, how long a value and a row are.
//
// Dialect and semantics.  JSON lines are what the reference's generator keeps per epoch -- serde_json::to_vec(event) + "\n"
// (flock/src/datasource/nexmark/generator.rs:79-93) --, CSV is what csv.hpp's A-CSV1..7 read back.  Checked against tests/text_encode_ref.py and, there,
// against json.dumps(ensure_ascii=False), tests/csv_ref.py and csv.reader(strict=True):
//   A-ENC1 JSON: a row is {"name":value,...}\n -- the columns in the given order, no white space, every row newline-terminated; zero rows are zero bytes.
//          Keys are escaped by A-ENC3, on the host;
//   A-ENC2 Int32 / Int64 / UInt64 print in their shortest decimal form (numtext.hpp A-NT2).  In JSON a Timestamp(ms) prints as the same integer (it is
//          Int64 at that boundary, as in the decoder); in CSV as 'YYYY-MM-DD HH:MM:SS[.mmm]' (A-NT3), which csv.hpp's timestamp_ms reads;
//   A-ENC3 a JSON string is "..." with serde_json's escapes: '"' -> \", '\' -> \\, 0x08 0x0C 0x0A 0x0D 0x09 -> \b \f \n \r \t, every other byte below 0x20 ->
//          \u00xx with lower-case hex; everything else verbatim -- 0x7F, '/', bytes >= 0x80 --, nothing checks UTF-8 (json.hip A-JSON7);
//   A-ENC4 NULL is `null` in JSON and an empty unquoted field in CSV, whatever the type.  Known loss: csv.hpp A-CSV6 reads an empty Utf8 field as '', so a
//          NULL Utf8 comes back as '';
//   A-ENC5 CSV: fields joined by the delimiter (any ASCII byte except '"', CR, LF, as in the decoder), every record ends in '\n'.  has_header writes one
//          record of the names first, each quoted by A-ENC6 (also when there are no rows);
//   A-ENC6 a CSV Utf8 value is quoted when it is empty or holds the delimiter, '"', LF or CR; inside quotes '"' is doubled; otherwise it is verbatim;
//   A-ENC7 a CSV record that would be empty -- a one-column table's NULL -- is written "": the decoder refuses blank lines and reads "" as NULL / '';
//   A-ENC8 refused before anything is launched: a Float64 column (no shortest-round-trip form on the device: numtext.hpp A-NT6), more than 64 columns,
//          a name that is empty or longer than 31 bytes -> FLOCKGPU_ERR_UNSUPPORTED naming the column; no columns, a bad delimiter, rows < 0 or
//          >= 2^31, a Utf8 column without offsets, an unknown type -> FLOCKGPU_ERR_INVALID;
//   A-ENC9 refused after the length pass, before the emit pass allocates or launches: an output of 2^31 - 16 bytes or more -> FLOCKGPU_ERR_UNSUPPORTED;
//          CSV only, a non-NULL timestamp outside the years 0000..9999 -> FLOCKGPU_ERR_INVALID naming the FIRST such record (1-based, the header counted)
//          and the column;
//   A-ENC10 the bytes depend on the columns alone, not on grid shape or batching; no byte at or past the end of an input buffer is read.
#pragma once
#include <cstdint>

#include "numtext.hpp"
#include "textslice_bits.hpp"

namespace flockgpu {

// (the values of include/flockgpu.h's FLOCKGPU_TEXT_*: the CSV decoder's numbering)
enum : int32_t { kTextInt32 = 0, kTextInt64 = 1, kTextUInt64 = 2, kTextFloat64 = 3, kTextTimestampMs = 4, kTextUtf8 = 5 };
enum class TextFormat : int32_t { Json = 0, Csv = 1 };

constexpr int kTextEncMaxCols = 64;
constexpr int kTextEncMaxName = 31;
constexpr int kTextEncPreWords = 48;   // the bytes in front of a value: ',"' + a name of 31 bytes that all escape to six + '":' = 190 bytes

namespace textenc {

// ---- byte classes, one byte ------------------------------------------------------------------------------------------------------------------------
// JSON: bytes an escape replaces; `long`: by the six bytes of \u00xx
FG_HD bool json_is_class(uint32_t b) { return b < 0x20u || b == 0x22u || b == 0x5Cu; }
FG_HD bool json_is_long(uint32_t b) { return b < 0x20u && !((0x3700u >> b) & 1u); }   // (0x3700: 0x08 0x09 0x0A 0x0C 0x0D, the short escapes)
FG_HD uint32_t json_extra(uint32_t b) { return json_is_class(b) ? (json_is_long(b) ? 5u : 1u) : 0u;}
// CSV: bytes that force quotes; '"' is also doubled
FG_HD bool csv_is_special(uint32_t b, uint32_t delim) { return b == delim || b == 0x22u || b == 0x0Au || b == 0x0Du; }

// What one byte of a JSON string becomes: the bytes in out[0 .. n), n = 1, 2 or 6
FG_HD uint32_t json_escape(uint32_t b, uint8_t *out) {
    if (!json_is_class(b)) {
        out[0] = (uint8_t)b;
        return 1u;
    }
    out[0] = (uint8_t)'\\';
    if (!json_is_long(b)) {
        out[1] = b == 0x22u ? (uint8_t)'"' : b == 0x5Cu ? (uint8_t)'\\' : b == 0x08u ? (uint8_t)'b' : b == 0x0Cu ? (uint8_t)'f' : b == 0x0Au ? (uint8_t)'n'
                 : b == 0x0Du ? (uint8_t)'r' : (uint8_t)'t';
        return 2u;
    }
    const uint32_t lo = b & 15u;
    out[1] = (uint8_t)'u';
    out[2] = (uint8_t)'0';
    out[3] = (uint8_t)'0';
    out[4] = (uint8_t)('0' + (b >> 4));
    out[5] = (uint8_t)(lo < 10u ? '0' + lo : 'a' + (lo - 10u));
    return 6u;
}

// ---- byte classes, four bytes of a little-endian dword: bit k speaks of byte k ---------------------------------------------------------------------
using slicebits::gather_bit7;   // bit 7 of every byte -> bits 0..3
// 0x80 in every byte of x that is zero (the carry-free test: the low seven bits are added to 0x7f inside their own byte)
FG_HD uint32_t zero_bytes(uint32_t x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }
FG_HD uint32_t equal_bytes(uint32_t w, uint32_t c) { return zero_bytes(w ^ (0x01010101u * c)); }

// JSON: *cls = the class bytes, *lng = those of them that take \u00xx
FG_HD void json_class4(uint32_t w, uint32_t *cls, uint32_t *lng) {
    const uint32_t ctl = zero_bytes(w & 0xe0e0e0e0u);   // below 0x20
    uint32_t l = 0;
    if (ctl) {   // (rare: generated text holds none)
        for (int k = 0; k < 4; ++k)
            if (json_is_long((w >> (8 * k)) & 0xffu)) l |= 1u << k;
    }
    *cls = gather_bit7(ctl | equal_bytes(w, 0x22u) | equal_bytes(w, 0x5Cu));
    *lng = l;
}
// CSV: *quo = the '"', *spc = the bytes that force quotes
FG_HD void csv_class4(uint32_t w, uint32_t delim, uint32_t *quo, uint32_t *spc) {
    const uint32_t q = equal_bytes(w, 0x22u);
    *quo = gather_bit7(q);
    *spc = gather_bit7(q | equal_bytes(w, delim) | equal_bytes(w, 0x0Au) | equal_bytes(w, 0x0Du));
}

// ---- lengths ---------------------------------------------------------------------------------------------------------------------------------------
// What the class pass keeps per Utf8 value, from the two counts of its bytes' classes:
//   JSON  the bytes the escapes add: one per class byte and four more per \u00xx;
//   CSV   the '"' (each doubled), and the two quotes when any special byte is there.  (The quotes of an EMPTY value are csv_utf8_len's.)
FG_HD uint32_t json_extra_of(uint32_t n_class, uint32_t n_long) { return n_class + 4u * n_long; }
FG_HD uint32_t csv_extra_of(uint32_t n_quote, uint32_t n_special) { return n_quote + (n_special ? 2u : 0u); }

FG_HD bool csv_utf8_quoted(uint32_t len, uint32_t extra) { return len == 0u || extra != 0u; }
FG_HD uint64_t json_utf8_len(uint32_t len, uint32_t extra) { return (uint64_t)len + extra + 2u; }
FG_HD uint64_t csv_utf8_len(uint32_t len, uint32_t extra) { return len == 0u ? 2u : (uint64_t)len + extra; }

// an integer's digits and sign; `bits`: the value's 64 bits (an Int32 sign-extended)
FG_HD uint32_t int_len(int32_t type, uint64_t bits) {
    if (type == kTextUInt64) return numtext::digits10_u64(bits);
    const int64_t v = (int64_t)bits;
    if (type == kTextInt32) return numtext::digits10_u32(v < 0 ? 0u - (uint32_t)v : (uint32_t)v) + (v < 0 ? 1u : 0u);
    return numtext::digits10_u64(v < 0 ? 0ull - (uint64_t)v : (uint64_t)v) + (v < 0 ? 1u : 0u);
}
// a value that is not Utf8 (a CSV timestamp: in range)
FG_HD uint32_t num_len(TextFormat f, int32_t type, bool valid, uint64_t bits) {
    if (!valid) return f == TextFormat::Json ? 4u : 0u;
    if (type == kTextTimestampMs) return f == TextFormat::Json ? int_len(kTextInt64, bits) : numtext_ts_len((int64_t)bits);
    return int_len(type, bits);
}
FG_HD uint64_t utf8_len(TextFormat f, bool valid, uint32_t len, uint32_t extra) {
    if (!valid) return f == TextFormat::Json ? 4u : 0u;
    return f == TextFormat::Json ? json_utf8_len(len, extra) : csv_utf8_len(len, extra);
}
// A row from the sum of its values' lengths and of the bytes in front of them ('{"name":' / ',"name":'; nothing / the delimiter): JSON closes with
// '}' and '\n', CSV with '\n' -- and a record that would be empty is '""' (A-ENC7)
FG_HD uint64_t row_len(TextFormat f, uint64_t pre_bytes, uint64_t value_bytes) {
    if (f == TextFormat::Json) return pre_bytes + value_bytes + 2u;
    return pre_bytes + value_bytes == 0u ? 3u : pre_bytes + value_bytes + 1u;
}

}  // namespace textenc
}  // namespace flockgpu
