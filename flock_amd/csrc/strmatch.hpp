// Utf8 LIKE / NOT LIKE and ordered comparisons (<, <=, >, >=) of a Utf8 column with a literal (strmatch.hip).  A kernel of its own per
// (column, pattern) leaf writes the leaf's TRUE bits in the flag-tile layout of scan.hpp -- one 32-bit word per lane and tile --, and the
// predicate program (pred.hpp) takes that word through a `Words` leaf that evaluates nothing: LIKE composes with every other leaf in the one
// pass, for 4 bytes per 32 rows, and pred_flag_kernel's register-tuned instances carry no string matcher.  NULL bits still come from the
// column's validity bytes, in the Words leaf.
//
// Assumptions (DESIGN.md section 3a repeats them):
//   A-L1  `%` matches any run of bytes, the empty run and newlines included.
//   A-L2  `_` matches exactly one UTF-8 code point: a byte that is not 10xxxxxx and the continuation bytes after it.  Values are valid UTF-8
//         (Arrow's contract); a `_` never matches in the middle of a code point.
//   A-L3  every other pattern byte matches itself; matching is case-sensitive and the WHOLE value must match.  The empty pattern matches the
//         empty string only; '%' matches every value that is not NULL.
//   A-L4  a NULL value gives NULL under LIKE and NOT LIKE alike (the filter drops the row); the result is never NULL otherwise.
//   A-L5  there is no escape character: a pattern that holds a backslash is refused (nothing in the reference writes one, and the Arrow
//         implementations disagree about it).
//   A-L6  this is the SQL meaning, which Arrow C++ implements (pyarrow.compute.match_like).  arrow-rs of the fork's era is believed to have turned the
//         pattern into an unquoted regex whose `.` does not match a newline; the fork's expressions/*.rs are not at hand to check (beside A-V3).
//   A-L7  ordered comparison is bytewise lexicographic, a proper prefix first: the order sort_rows gives Utf8.  A NULL value gives NULL.
//
// Matching: the pattern is cut at every `%` into pieces of literal bytes and `_` (k `%` give k + 1 pieces, empty ones included).  Without a
// `%` the value must match the one piece exactly.  Otherwise the first piece is anchored at the value's start, the last at its end (matched
// backwards), and every piece between them is taken at its LEFTMOST position at or after the end of the piece before it -- sufficient,
// because an earlier match never shrinks what is left for the later pieces.
//
// Limits: a pattern (or a comparison literal) of up to kStrMaxPattern bytes with up to kStrMaxPieces - 1 `%`.  The compiled pattern travels
// as a kernel argument, so the predicate program's literal pool (kPredLitPool) does not bound it.
#pragma once
#include <string>

#include "relops.hpp"

namespace flockgpu {

constexpr int kStrMaxPattern = 128;
constexpr int kStrMaxPieces = 17;
// bytes of a value range one round of the `%needle%` kernel holds in LDS (tests/test_plan_like.py mirrors this to place needles across a round's edge)
constexpr int kStrStageBytes = 16384;

enum class StrOp : uint8_t { Like = 0, Lt = 2, Le = 3, Gt = 4, Ge = 5 };   // (the comparisons: CmpOp's numbers)

struct StrPattern {
    uint8_t bytes[kStrMaxPattern];       // the pieces' bytes back to back (`%` removed); the comparison literal
    uint8_t piece_off[kStrMaxPieces + 1];
    int32_t n_pieces;                    // Like: k + 1
    int32_t len;                         // bytes used
    uint8_t op;                          // StrOp
    uint8_t has_underscore;
    uint8_t pad[2];
};

// false: beyond the limits above (*why says which)
bool strmatch_compile_like(const std::string &pattern, StrPattern *out, std::string *why);
bool strmatch_compile_cmp(const std::string &literal, int cmp_op, StrPattern *out, std::string *why);

// words[tile * 256 + thread]: bit it * 4 + j = the leaf is TRUE for the row of that lane slot (flag-tile layout, tiles of rows [0, rows) from row 0).
// *out_words: ctx-owned (arena key `name`).  No host wait.
int strmatch_words(flockgpu_ctx *ctx, const char *name, const DevColumn &col, int64_t rows, const StrPattern &pat, uint32_t **out_words);

}  // namespace flockgpu
