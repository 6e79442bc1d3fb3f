// UnionExec (union.hip; plan.hip exec_union): UNION ALL -- the rows of input 0, then input 1's, and so on.  Nothing is compared, hashed or counted:
// like the cross join the operator is OUTPUT-bound, one read and one write per value, so its kernels follow the recipe cross.hip and textsel.hip
// measured: every lane assembles whole 16-byte chunks of the OUTPUT and stores them aligned, non-temporal.  What is new are the SEAMS between the
// inputs (input k + 1 begins wherever input k ended: at any misalignment of the 16 bytes), inputs that arrive as ROW LISTS (a filter directly under
// the union: its surviving rows are read in place, src[via[i]], never taken first and copied second) and MIXED VALIDITY (inputs with validity bytes
// beside inputs without).
//
// Plan dialect: `"execution_plan": "union_exec"` with `"inputs": [plan, ...]` and optionally `schema`.  The fork's typetag name cannot be checked (its
// DataFusion source is not under the reference): it follows the naming of every tag that has been seen.  One input is an identity; a union directly
// under a union -- also through the transparent nodes (coalesce_batches_exec, coalesce_partitions_exec, merge_exec, a round-robin repartition) -- is
// flattened at create.  No input, or more than kUnionMaxInputs after flattening, is refused by name at create / explain.
//
// Semantics -- like cross.hpp A-X1..6 ASSUMPTIONS restated from upstream DataFusion ~5/6 (UnionExec), checked against tests/union_ref.py:
//   A-U1 schema    names come from input 0; every input has input 0's column count and, per column, its type and is_ts -- otherwise the plan is
//                  refused at create / explain, the message names the input, the column and both types.  A column is nullable when it is in any
//                  input.  A serialised `schema` that disagrees in count or types is refused by name;
//   A-U2 rows      all rows of input 0 in their order, then input 1's, ... (upstream concatenates the inputs' partitions in input order; batch
//                  boundaries are unobservable at this boundary);
//   A-U3 NULLs     travel verbatim.  The output column carries validity bytes exactly when some input's column does; inputs without contribute ones;
//                  an input's all_null column contributes zero validity, zero values and empty strings; a column that is all_null in EVERY input
//                  stays all_null;
//   A-U4 empty     an empty input contributes nothing; every input empty: zero rows with the full schema;
//   A-U5 pruning   only the columns some ancestor reads (Node::required) are produced; COUNT(*) over a union produces none, its row count is the sum
//                  of the inputs' row counts;
//   A-U6 limits    2^31 rows or more, or 2^31 bytes or more in an output Utf8 column, are refused at execute (FLOCKGPU_ERR_UNSUPPORTED, the node
//                  named) before anything of the result is allocated or launched;
//   A-U7 leaves    Exec::resolve_leaf lets an unfed leaf read the fed leaf of the same columns, but only for the columns that leaf also `needed`:
//                  `SELECT auction FROM bid WHERE .. UNION ALL SELECT bidder FROM bid WHERE ..` would scan an empty second branch silently.  In a
//                  plan that contains a union_exec -- and only there -- leaves with identical field lists get the OR of their `needed` masks (and
//                  the AND of their null_droppable marks: a row one branch could drop is a row of the other) at create.
//   Still open: an aggregate or filter that reads a union without materialising it; a gather-concat for text (the Utf8 columns of an input with a
//   row list are taken ONCE by the existing take, for the columns somebody reads, and then concatenated).
//
// Kernels.  Up to kUnionSources sources per launch travel BY VALUE as {src, via, valid, first output element, elements} (as textsel passes its
// sources); more inputs go in rounds of kUnionSources, each round writing its own range [lo, hi) of the output -- a chunk two rounds share is written
// element by element by both, each its own elements.  A lane finds the source of its first element by comparing against the table and steps to the
// next source at a seam: a chunk that straddles a seam takes its elements from both sides.  A workgroup makes kUnionTileChunks chunks.
//   union_fixed_kernel    4-byte and 8-byte values.  A source without a row list is a streaming copy at rebased alignment (aligned 16-byte loads,
//                         shifted); a source with one is read as src[via[i]] in place.  An all_null source (src null) gives zeros;
//   union_valid_kernel    the sibling at width 1 over the `valid` pointers, through `via` where there is one; no validity: ones; all_null: zeros;
//   union_offsets_kernel  Utf8 offsets, every source's rebased by the bytes in front of it (64 bits, narrowed after A-U6); entry n_out = the total;
//   union_bytes_kernel    the sources' byte buffers one after the other: 16-byte chunks at rebased alignment (aligned dword loads funnel-shifted),
//                         the chunk at a seam -- and a source's last fifteen bytes -- byte by byte from both sides.
// The host knows every input's row count and every Utf8 column's byte total without a wait (DevColumn::bytes).  Results do not depend on grid shape or
// batching: nothing accumulates, every output element is a function of its index.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#include "relops.hpp"   // (first: divmagic.hpp's host / device qualifiers are the HIP runtime's)
#endif
#include "divmagic.hpp"

namespace flockgpu {

constexpr int kUnionTileChunks = 1024;   // 16-byte output chunks of one workgroup: four per lane
constexpr int kUnionSources = 16;        // sources of one launch
constexpr int kUnionMaxInputs = 64;      // inputs of one union_exec after flattening
constexpr int64_t kUnionMaxRows = int64_t(1) << 31;    // A-U6: the output's rows below this
constexpr int64_t kUnionMaxBytes = int64_t(1) << 31;   // A-U6: every output Utf8 column below this

// One source of a launch.  `first` / `count` are output ELEMENTS: rows for values, validity bytes and offsets, bytes for union_bytes_kernel.
// Sources of a table are non-empty, in output order and adjacent: first[k + 1] = first[k] + count[k].
struct UnionSource {
    const void *src;        // values (Utf8: bytes; union_offsets_kernel: offsets); null: an all_null source
    const int32_t *via;     // row list (null: rows 0 .. count - 1 themselves)
    const uint8_t *valid;   // validity bytes (null: every row valid)
    uint32_t first;
    uint32_t count;
};
struct UnionSources {
    UnionSource s[kUnionSources];
    uint64_t base[kUnionSources];   // union_offsets_kernel: the bytes in front of the source
    int32_t n;                      // sources in use, >= 1
    uint32_t lo, hi;                // the launch's output range: s[0].first and s[n - 1].first + s[n - 1].count
};

// ---- host-callable index helpers (plain C++: tests/cpp/union_index_test.cpp checks them against their definitions on the CPU)
// the source output element e belongs to: the last k with s[k].first <= e (e inside [lo, hi))
FLOCKGPU_HD int union_source_of(const UnionSources &S, uint32_t e) {
    int k = 0;
    for (int i = 1; i < kUnionSources; ++i)
        if (i < S.n && S.s[i].first <= e) k = i;
    return k;
}
// how many of the `width` elements from e on lie in source k (e inside it): `width` when no seam falls into the chunk, else the seam's position
FLOCKGPU_HD uint32_t union_seam_in_chunk(const UnionSources &S, int k, uint32_t e, uint32_t width) {
    const uint64_t end = (uint64_t)S.s[k].first + S.s[k].count;
    return end - e < width ? (uint32_t)(end - e) : width;
}
// entry i of a source's offsets, rebased by the bytes in front of the source (a source's own offsets begin at 0)
FLOCKGPU_HD uint64_t union_rebased_offset(uint64_t base, uint64_t off_i) { return base + off_i; }
// A-U6: the sum of `n` non-negative counts; false -- and *out = 0 -- when it reaches `limit` (no overflow for any int64 counts)
inline bool union_sum_ok(const int64_t *counts, int n, int64_t limit, int64_t *out) {
    int64_t sum = 0;
    *out = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t c = counts[i] > 0 ? counts[i] : 0;
        if (c >= limit || sum + c >= limit) return false;
        sum += c;
    }
    *out = sum;
    return true;
}
inline bool union_rows_ok(const int64_t *rows, int n, int64_t *out) { return union_sum_ok(rows, n, kUnionMaxRows, out); }
inline bool union_bytes_ok(const int64_t *bytes, int n, int64_t *out) { return union_sum_ok(bytes, n, kUnionMaxBytes, out); }

#ifdef __HIPCC__
// One input's column as union_column sees it: a plain column (`via` null) or one read through a row list; Utf8 columns arrive taken (via null).
struct UnionInput {
    DevColumn col;
    const int32_t *via = nullptr;
    int64_t rows = 0;
};
// out = the inputs' columns one after the other (A-U2, A-U3): values, validity bytes, Utf8 offsets and bytes; buffers live in the ctx arena under
// `name`.  The inputs share `col.type`; the row total and a Utf8 result's bytes are checked against A-U6 before anything is allocated.  Launches only.
int union_column(flockgpu_ctx *ctx, const char *name, const UnionInput *in, int n_in, DevColumn *out);
#endif

}  // namespace flockgpu
