// Utf8-VALUED expressions of ProjectionExec (textsel.hip): text literals, Utf8 columns and CASE whose branches are text.  The numeric evaluator
// (valprog.hpp) stays what it was: the expression is lowered on the host (plan.hip text_compile) into
//   a SELECTOR  the same CASE with every text branch replaced by the index of its SOURCE (0 .. K - 1) and NULL kept NULL: an Int32 program of
//               the existing interpreter, nested CASE as nested Select.  A bare literal or column has no selector;
//   a SOURCE TABLE (TextSources, passed by value): K entries, each a literal (offset and length in a pool of at most kTextMaxLiteralBytes), a
//               Utf8 column of the input (offsets, bytes, validity bytes) or a SLICE of such a column (textslice.hpp: per row the begin and end of the
//               value inside the column's bytes, in place of its two offsets);
// and two kernels turn (selector, table) into an ordinary Utf8 column -- int32 offsets, bytes, validity bytes:
//   length pass  per row the selected source's length (a literal's from the table in LDS, a column's from its two offsets) -> one byte count per
//                wave for the tile scan (scan.hpp), and the result's validity bytes where a NULL can occur;
//   -- tile scan; the total goes to pinned memory; the host waits once, checks it against 2^31 and sizes the byte buffer --
//   emit pass    offsets (one aligned 16-byte store per lane: a lane owns four consecutive rows) and bytes.  A tile whose bytes fit kTextStageBytes
//                (literals, short values) is assembled in LDS and streamed out as aligned 16-byte chunks, the two chunks it shares with its
//                neighbour tiles byte by byte (textsel_emit_kernel); every larger tile -- long column values, up to single values of any length --
//                goes through the take's chunk-wise copy for long values (utf8_chunks.hpp, shared with gather.hip utf8_emit_long_kernel) over
//                the tile's (address, length) list in LDS (textsel_emit_long_kernel): every lane builds whole 16-byte output chunks.
// A projection of literals alone (NEXMark q14's bid_time_type) reads nothing but the selector; a bare literal is one fill.
//
// Dialect and semantics (DataFusion ~6 CaseExpr / Literal; like valprog.hpp's A-V / A-F lists ASSUMPTIONS, not reference-held vectors -- checked
// against tests/text_expr_ref.py and, there, against pyarrow.compute.case_when):
//   A-T1 a text-valued expression is a Utf8 literal ({"Utf8": null}: a NULL of type Utf8), a Utf8 column (a cast_expr to Utf8 may sit in front),
//        a cast_expr / try_cast_expr to Utf8 of an integer or Timestamp(ms) value (A-T7), or a case_expr whose THEN / ELSE branches are text-valued or untyped NULL literals (nested CASE counts).  Its static type is Utf8; leading
//        NULL branches do not hide it.  A CASE that mixes text and numeric branches is refused ("CASE branches of different types");
//   A-T2 CASE picks the first WHEN that is TRUE (NULL and FALSE are not), else ELSE, else NULL; `CASE WHEN cond` and `CASE base WHEN value` are
//        both taken; conditions, base and value are what the general evaluator takes (numeric, Timestamp, scalar functions, IS NULL, IN, Kleene
//        AND / OR / NOT) and every one of them is evaluated for every row (A-V7: a zero divisor in a branch that is never chosen fails the call);
//   A-T3 '' is a value, not NULL; a chosen column whose row is NULL gives NULL; bytes are copied verbatim (no validation, no normalisation);
//        the result is nullable;
//   A-T4 taken as a projection_exec output column and, through the projection computed_column puts underneath, as a GROUP BY key, an ORDER BY
//        key, the argument of COUNT / COUNT(DISTINCT) and a DISTINCT column -- hence under and over filters, joins, sorts, limits and in stage
//        plans.  The result is an ordinary Utf8 column every consumer reads unchanged; its bytes do not depend on batching or grid shape;
//   A-T5 refused by name at create / explain: more than kTextMaxSources distinct sources (literals plus columns) in one expression, more than
//        kTextMaxLiteralBytes bytes of (distinct) literals in one expression.  Refused at execute: a result of 2^31 bytes or more, checked on
//        the published total before any byte is written.
//   A-T6 the slice functions split_part / left / right / ltrim / rtrim / btrim of a Utf8 column (textslice.hpp A-SL1..A-SL8) are text-valued
//        expressions too: one slice expression is one source, identical ones count once.
//   A-T7 CAST(x AS Utf8) / TRY_CAST(x AS Utf8) of an Int32 / Int64 / UInt64 / Timestamp(ms) column or numeric expression (numtext.hpp A-NT1..A-NT7) is a
//        text-valued expression too.  The cast is computed into an ordinary Utf8 column first (numtext.hip) and enters the table as a COLUMN source:
//        one source, identical casts once; a bare projected cast is that column itself.  A Float64, Boolean or literal operand is refused by name.
//   Still refused, as before: a Utf8 column or literal inside a condition or under an operator, LIKE inside a computed expression, the other
//   text-producing scalar functions (substr, lower, upper, trim, concat, ...), Boolean projections, hash partitioning on a computed expression,
//   MIN / MAX of text.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "numtext.hpp"
#include "textnum.hpp"
#include "relops.hpp"

namespace flockgpu {

constexpr int kTextMaxSources = 16;
constexpr int kTextMaxLiteralBytes = 1024;
constexpr int kTextTile = 1024;          // rows of a workgroup: four consecutive rows per lane
constexpr int kTextStageBytes = 16384;   // the LDS stage of the emit pass: a tile of more bytes takes the chunk-wise kernel

struct TextSource {
    const int32_t *offsets;   // column source; null: a literal
    const uint8_t *bytes;
    const uint8_t *valid;     // column source with NULLs: one byte per row
    uint32_t lit_off, lit_len;   // literal: where it lies in the pool (a multiple of four), its length
    const int32_t *begin, *end;  // a slice of the column: row i's value is bytes [begin[i], end[i]); null: [offsets[i], offsets[i + 1])
};
struct TextSources {
    TextSource src[kTextMaxSources];
    uint32_t pool[(kTextMaxLiteralBytes + 4 * kTextMaxSources) / 4];   // the literals, each from a 4-byte boundary on
    int32_t k = 0;
    int32_t n_cols = 0;   // column sources among the k
    int32_t n_slices = 0; // slices among the column sources
};

// Host-side assembly: every add returns the source's index (a literal or column that is already there: its index), -1 when the table is full.
struct TextTable {
    TextSources s{};
    uint32_t pool_used = 0;
    std::vector<std::string> lits;   // by source index ("" for a column)
    std::vector<std::string> slice_keys;   // by source index: the slice expression's text ("" for anything else)
    int add_literal(const std::string &v) {
        for (int i = 0; i < s.k; ++i)
            if (!s.src[i].offsets && lits[(size_t)i] == v) return i;
        if (s.k >= kTextMaxSources || pool_used + v.size() > sizeof(s.pool)) return -1;
        TextSource &t = s.src[s.k];
        t = TextSource{nullptr, nullptr, nullptr, pool_used, (uint32_t)v.size(), nullptr, nullptr};
        std::memcpy(reinterpret_cast<uint8_t *>(s.pool) + pool_used, v.data(), v.size());
        pool_used = (pool_used + (uint32_t)v.size() + 3u) & ~3u;
        lits.push_back(v);
        slice_keys.emplace_back();
        return s.k++;
    }
    int add_column(const DevColumn &c) {
        for (int i = 0; i < s.k; ++i)
            if (s.src[i].offsets == c.offsets && s.src[i].bytes == c.values && s.src[i].valid == c.valid && !s.src[i].begin) return i;
        if (s.k >= kTextMaxSources) return -1;
        s.src[s.k] = TextSource{c.offsets, static_cast<const uint8_t *>(c.values), c.valid, 0, 0, nullptr, nullptr};
        lits.emplace_back();
        slice_keys.emplace_back();
        ++s.n_cols;
        return s.k++;
    }
    // the slice expression `key` (its text: identical expressions are one source) already in the table: its index, else -1
    int find_slice(const std::string &key) const {
        for (int i = 0; i < s.k; ++i)
            if (s.src[i].begin && slice_keys[(size_t)i] == key) return i;
        return -1;
    }
    int add_slice(const DevColumn &c, const int32_t *begin, const int32_t *end, const std::string &key) {
        if (s.k >= kTextMaxSources) return -1;
        s.src[s.k] = TextSource{c.offsets, static_cast<const uint8_t *>(c.values), c.valid, 0, 0, begin, end};
        lits.emplace_back();
        slice_keys.push_back(key);
        ++s.n_cols;
        ++s.n_slices;
        return s.k++;
    }
};

// out = for every row i the value of source sel[i] (sel null: source 0 for every row); a row whose sel_valid byte is 0 (sel_valid may be null) or
// whose chosen column holds a NULL there is NULL.  No source at all: every row NULL.  Offsets, bytes and validity live in the ctx arena under
// `name`.  One host wait (the byte total); none for a bare literal or an empty result.
int text_select(flockgpu_ctx *ctx, const char *name, const TextSources &srcs, const int32_t *sel, const uint8_t *sel_valid, int64_t rows, DevColumn *out);

// CAST(`in` AS Utf8) (numtext.hip; numtext.hpp A-NT1..A-NT7): `in` an Int32 / Int64 / UInt64 column, a Timestamp(ms) one when in.is_ts.  A NULL row gives
// a NULL; a timestamp outside the years 0000..9999 gives a NULL when `try_cast`, else the call fails naming `who` (the expression's tag).  Offsets, bytes
// and validity live in the ctx arena under `name`.  One host wait (the byte total, and with it the flag word).
int num_to_text(flockgpu_ctx *ctx, const char *name, const DevColumn &in, int64_t rows, bool try_cast, const char *who, DevColumn *out);

// CAST(`col` AS Int32 / Int64 / UInt64 / Timestamp(ms)) of a Utf8 column (textnum.hip; textnum.hpp A-TN1..A-TN6), or -- `range_begin` / `range_end` given --
// of the per-row byte ranges of a text slice of it (textslice.hpp).  `out`: a nullable column of the target type, values and validity bytes in the ctx
// arena under `name`; a NULL row gives a NULL, a value that does not parse a NULL as well and -- unless `try_cast` -- a 1 in *h_fail, a word of pinned
// host memory the kernel stores to.  Launches only: the caller reads *h_fail after its next wait on the stream (the evaluator's, for its own failure
// word).  Zero rows launch nothing.
int text_to_num(flockgpu_ctx *ctx, const char *name, const DevColumn &col, int64_t rows, TextNumKind kind, bool try_cast, const int32_t *range_begin, const int32_t *range_end,
                DevColumn *out, const uint32_t **h_fail);

}  // namespace flockgpu
