// CrossJoinExec (cross.hip; plan.hip exec_cross): every row of the left input paired with every row of the right one.  There are no keys, nothing
// is hashed and nothing is compared: the operator is OUTPUT-bound -- it writes L x R values per column from sources that are small or read once --
// so it builds no pair lists (two int32 row lists of L x R entries, written, read again and gathered through, are what an inner join on a constant
// key pays) and produces every column directly:
//   left columns   = REPEAT  source value i, R times in a row            out[i * R + j] = src[i]
//   right columns  = TILE    the whole source column, L times over       out[i * R + j] = src[j]
// A side that arrives with a row list (a filter directly under the join) is TAKEN ONCE for the columns somebody reads -- L or R rows, the small
// cost -- and the result is replicated; the kernels never read through a row list.
// A side of exactly ONE row (a global aggregate's row, known only at execute): the OTHER side's columns are that side's table itself -- no kernel,
// no copy (a row list is taken once) -- and the one row's columns are FILLS, the repeat of one source row.
//
// Plan dialect: `"execution_plan": "cross_join_exec"` with `left`, `right` and optionally `schema`.  The fork's typetag name cannot be checked (its
// DataFusion source is not under the reference): it follows the naming of every tag that has been seen (hash_join_exec, window_agg_exec).  `on`,
// `join_type`, `mode`, `random_state`, where present, are ignored.
//
// Semantics -- like relops.hpp A-S1..6 and textsel.hpp A-T1..5 ASSUMPTIONS restated from upstream DataFusion ~6, checked against
// tests/cross_join_ref.py:
//   A-X1 schema    the left input's columns followed by the right input's; names, types, is_ts and nullability unchanged.  A serialised schema whose
//                  column count or types are not left ++ right is refused by name at create / explain;
//   A-X2 rows      every (left row i, right row j) exactly once, L x R rows; pair (i, j) is output row i * R + j (left-major) -- what CrossJoinExec
//                  yields when its right side arrives as one batch (recalled from upstream, NOT checkable here: an assumption).  Batch boundaries
//                  are unobservable at this boundary: the order is the same however the inputs were fed;
//   A-X3 NULLs     nothing is compared: a NULL travels verbatim (validity bytes are repeated / tiled with the values); a column that is nothing
//                  but NULLs (all_null) stays so;
//   A-X4 empty     L = 0 or R = 0: zero rows with the full schema;
//   A-X5 pruning   only the columns some ancestor reads (Node::required) are produced; COUNT(*) over a cross join produces no column at all, its
//                  row count is L x R;
//   A-X6 limits    L x R >= 2^31 rows is refused at execute (FLOCKGPU_ERR_UNSUPPORTED, the message names the node and both row counts), and so
//                  is an output Utf8 column of 2^31 bytes or more -- both before anything of the result is allocated or launched (a side's row
//                  list is taken first: a taken column's byte total is what the byte check reads).
//   Still refused: Left / Right / Full joins, a join filter inside the operator, a stage cut at a cross join.
//
// Kernels.  Every lane assembles whole 16-byte chunks of the OUTPUT and stores them aligned, non-temporal (the store path: eight 4-byte accesses
// per lane cost a segment per lane where 16-byte ones do not, README round 6; textsel_fill_kernel reaches 0.82 of the peak that way).  A chunk of
// a repeat straddles source rows when R is no multiple of the chunk's elements, a chunk of a tile wraps from source row R - 1 to row 0: the lane
// takes quotient and remainder of its first element by R once (divmagic.hpp's reciprocal, no hardware divide) and steps them.  A workgroup makes
// kCrossTileChunks chunks: kCrossTileChunks * 16 / width rows of a column.
//   cross_repeat_kernel / cross_tile_kernel   4-byte and 8-byte values and validity bytes; the FILL (one source row) is the repeat's L = 1 and
//                                             shows in the profile as cross_fill_kernel -- one kernel, no third fill;
//   cross_offsets_kernel                      Utf8 offsets in closed form, four per lane:  repeat out_off[i * R + j] = R * off[i] + j * len[i],
//                                             tile out_off[i * R + j] = i * total + off[j]; computed in 64 bits, narrowed after the A-X6 check;
//   cross_tile_bytes_kernel                   the source byte buffer L times over: a streaming copy in 16-byte chunks at rebased alignment (aligned
//                                             dword loads funnel-shifted; the chunk that wraps goes byte by byte);
//   cross_repeat_bytes_kernel                 every value's bytes R times: utf8_chunks.hpp's chunk-wise emit over tiles of kCrossTextTile OUTPUT
//                                             values, whose positions are the closed form above -- no length pass, no scan, no wait.
// The host knows every source column's byte total without a wait (DevColumn::bytes: a leaf's is kept at feed, a taken column's arrives from the
// take's scan).  Results do not depend on grid shape or batching: nothing accumulates, every output element is a function of its index.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#include "relops.hpp"   // (first: divmagic.hpp's host / device qualifiers are the HIP runtime's)
#endif
#include "divmagic.hpp"

namespace flockgpu {

constexpr int kCrossTileChunks = 1024;   // 16-byte output chunks of one workgroup (fixed-width, validity, offsets and tiled bytes): four per lane
constexpr int kCrossTextTile = 1024;     // OUTPUT values of one workgroup of cross_repeat_bytes_kernel: four per lane
constexpr int64_t kCrossMaxRows = int64_t(1) << 31;    // A-X6: L x R below this
constexpr int64_t kCrossMaxBytes = int64_t(1) << 31;   // A-X6: every output Utf8 column below this

// ---- host-callable index helpers (plain C++: tests/cpp/cross_index_test.cpp checks them against `/` and `%` and the definitions above on the CPU)
// quotient and remainder of n by m.d through divmagic.hpp's reciprocal
FLOCKGPU_HD void cross_divmod(uint32_t n, const UMod32 &m, uint32_t *q, uint32_t *r) {
    const uint32_t rem = umod32_apply(n, m);
    uint32_t quo;
    if (m.magic == 0) {
        quo = n >> m.shift;
    } else {
        const uint32_t hi = (uint32_t)(((uint64_t)n * m.magic) >> 32);
        quo = m.add ? ((((n - hi) >> 1) + hi) >> m.shift) : (hi >> m.shift);
    }
    *q = quo;
    *r = rem;
}
// L x R as a row count: false when it reaches 2^31 (A-X6); no overflow for any two non-negative int64 counts
inline bool cross_rows_ok(int64_t l, int64_t r, int64_t *out) {
    *out = 0;
    if (l <= 0 || r <= 0) return true;
    if (l >= kCrossMaxRows || r >= kCrossMaxRows || l > (kCrossMaxRows - 1) / r) return false;
    *out = l * r;
    return true;
}
// bytes of a Utf8 column of `bytes` source bytes replicated `times` times: false when they reach 2^31
inline bool cross_bytes_ok(int64_t bytes, int64_t times, int64_t *out) {
    *out = 0;
    if (bytes <= 0 || times <= 0) return true;
    if (bytes >= kCrossMaxBytes || times >= kCrossMaxBytes || bytes > (kCrossMaxBytes - 1) / times) return false;
    *out = bytes * times;
    return true;
}
// where output value (i, j) of a repeated / tiled Utf8 column starts (off_i = off[i], len_i = off[i + 1] - off[i]; total = off[rows])
FLOCKGPU_HD uint64_t cross_repeat_offset(uint64_t times, uint32_t j, uint64_t off_i, uint64_t len_i) { return times * off_i + (uint64_t)j * len_i; }
FLOCKGPU_HD uint64_t cross_tile_offset(uint64_t total, uint32_t i, uint64_t off_j) { return (uint64_t)i * total + off_j; }

#ifdef __HIPCC__
// out = every one of src's `rows` values `times` times in a row (rows * times rows): values, validity bytes, Utf8 offsets and bytes; buffers live in
// the ctx arena under `name`.  rows * times and a Utf8 result's bytes are checked against A-X6 before anything is allocated.  Launches only.
int cross_repeat(flockgpu_ctx *ctx, const char *name, const DevColumn &src, int64_t rows, int64_t times, DevColumn *out);
// out = src's `rows` values as a whole, `times` times over.
int cross_tile(flockgpu_ctx *ctx, const char *name, const DevColumn &src, int64_t rows, int64_t times, DevColumn *out);
#endif

}  // namespace flockgpu
