// Text slice functions (textslice.hip): split_part, left, right, ltrim, rtrim, btrim -- the text-producing scalar functions whose result is a
// CONTIGUOUS SLICE of their argument.  They need no new bytes, only a choice of bytes the column already holds: per row a (begin, end) pair of
// absolute byte positions in the column's byte buffer, which text_select (textsel.hpp) then reads as one more kind of source.  A nested call
// (btrim(split_part(x, ',', 2))) takes the inner call's (begin, end) in place of the row's offsets: one launch per call over the same bytes, one emit.
//
// Two kernels find the pairs:
//   text_slice_stream_kernel   every case whose byte class is decided BYTEWISE: a one-byte delimiter (class: the byte equals it), left / right
//                        (class: the byte begins a code point), a trim set of ASCII characters (class: the byte is not in the set).  The shape of
//                        utf8_chars_kernel (strlen.hip): a workgroup takes kSliceRows consecutive rows and streams the contiguous byte range they
//                        span in rounds of kSliceRoundBytes, every 16 bytes with ONE load at an aligned address (the partial first and last chunk
//                        byte by byte: nothing outside the rows is read); a lane reduces its chunk in registers to a 16-bit class mask and stages the
//                        MASK in LDS; after the barrier a lane takes rows and finds, among the mask words its row covers (read as aligned 64-bit
//                        words), the k-th set bit of the row -- popcount per word, a select inside the word (textslice_bits.hpp) -- or the last set
//                        bit.  A row that straddles rounds carries its running count in LDS; a row longer than a round is just more words.
//                          split_part(s, d, n)   begin = one past the (n - 1)-th delimiter (n = 1: the row's start), end = the n-th delimiter (fewer:
//                                                the row's end; fewer than n - 1: '')
//                          ltrim                 begin = the first set bit (none: the row's end)
//                          rtrim                 end = one past the last set bit (none: the row's start)
//                          btrim                 both
//                          left(s, n >= 0)       end = the (n + 1)-th lead byte (fewer: the row's end)
//                          right(s, n < 0)       begin = the (|n| + 1)-th lead byte (fewer: the row's end)
//                          left(s, n < 0) / right(s, n > 0)   count from the END: k = (the row's code points) - |n| is PER ROW, from utf8_lengths over
//                                                the same range; k <= 0: the row's start, else the (k + 1)-th lead byte.  The kernel takes a constant
//                                                k or a per-row array.
//   text_slice_general_kernel  everything else -- a delimiter of 2 to 16 bytes (greedy leftmost matching), a trim set with a non-ASCII code point
//                        (code point by code point from either end): one lane per row walks its value in global memory.  For completeness; not tuned.
// No byte is copied and the host never waits.
//
// Dialect and semantics (DataFusion ~6 string_expressions.rs / unicode_expressions.rs; their source is not under the reference, so -- like valprog.hpp's
// A-F list -- ASSUMPTIONS, checked against tests/text_slice_ref.py and, there, against pyarrow.compute):
//   A-SL1 scalar_function_expr named split_part, left, right, ltrim, rtrim or btrim (case-insensitive); return_type, where present, is Utf8.  The
//         value argument is a Utf8 column or another slice function of one (a cast_expr to Utf8 may sit in front of either), nested at most
//         kSliceMaxDepth deep -- and a cast_expr / try_cast_expr to Utf8 of an integer or Timestamp(ms) value (numtext.hpp A-NT1..A-NT7) counts as such a
//         column: left(CAST(b_date_time AS Utf8), 10) is NEXMark q10's date; every other argument is a literal (a cast to the literal's own type may sit in front of it).  Refused by name at create /
//         explain: a column or computed n / delim / chars, a NULL literal argument, a literal, CASE or other text expression as the value argument,
//         a wrong argument count, deeper nesting, and the limits of A-SL2 / A-SL5;
//   A-SL2 split_part(s, delim, n): field n (1-based) of s cut at every non-overlapping, leftmost occurrence of delim ('aaa' cut at 'aa': 'a' is field
//         2); '' when there are fewer fields.  delim holds 1 to kSliceMaxDelimBytes bytes -- an empty one is refused (Rust's split("") and Postgres
//         disagree) --, n is an integer literal within Int32 and n <= 0 is refused (upstream fails the call);
//   A-SL3 left(s, n): n >= 0 the first n code points, n < 0 all but the last |n|; '' when nothing is left.  n within Int32;
//   A-SL4 right(s, n): n > 0 the last n code points, n < 0 all but the first |n|, n = 0 gives '';
//   A-SL5 ltrim(s) / rtrim(s) / btrim(s) strip U+0020 only (a tab stays); ltrim(s, chars) and its siblings strip any code point of chars, which holds
//         at most kSliceMaxTrimChars code points; an empty chars strips nothing;
//   A-SL6 a code point is a byte that is not 10xxxxxx plus the continuation bytes behind it (A-L2); bytes are copied verbatim (no validation);
//   A-SL7 NULL in gives NULL out; '' is a value; no function fails a call;
//   A-SL8 such a node is a text-valued expression (A-T1): a projected column, a THEN / ELSE branch of a text CASE, and through computed_column a
//         GROUP BY / ORDER BY / DISTINCT key and the argument of COUNT / COUNT(DISTINCT).  One slice expression is ONE source of the table (A-T5);
//         identical slice expressions count once.  The result is never larger than its argument;
//   Not taken: substr, lower, upper, trim, concat and the other text-producing functions (refused as before), column-valued n / delim / chars,
//   a slice as the argument of char_length / LIKE / a comparison.
#pragma once
#include <string>

#include "relops.hpp"

namespace flockgpu {

constexpr int kSliceRows = 1024;            // rows of a workgroup of the streaming kernel
constexpr int kSliceRoundBytes = 32768;     // bytes of a round: eight 16-byte loads in flight per lane
constexpr int kSliceMaxDelimBytes = 16;
constexpr int kSliceMaxTrimChars = 16;
constexpr int kSliceMaxDepth = 4;

enum class SliceFn : uint8_t { SplitPart, Left, Right, Ltrim, Rtrim, Btrim };

struct SliceSpec {
    SliceFn fn = SliceFn::SplitPart;
    int32_t n = 0;       // split_part: the field; left / right: the count
    std::string arg;     // split_part: the delimiter; the trims: the characters (one-argument form: " ")
};

// true: the streaming kernel takes `spec` (its class is decided bytewise); false: the general kernel
bool text_slice_streams(const SliceSpec &spec);

// begin[i], end[i] for rows 0 .. rows - 1 of `col` (Int32 arrays in the ctx arena under `name`): off[i] <= begin[i] <= end[i] <= off[i + 1].  With
// in_begin / in_end (both or neither) the call slices [in_begin[i], in_end[i]) instead of the whole value.  A NULL row's pair is computed from whatever
// its offsets span.  No host wait.
int text_slice(flockgpu_ctx *ctx, const char *name, const DevColumn &col, int64_t rows, const SliceSpec &spec, const int32_t *in_begin, const int32_t *in_end,
               int32_t **out_begin, int32_t **out_end);

}  // namespace flockgpu
