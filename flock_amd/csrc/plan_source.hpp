// Device-side ingest of a plan leaf (plan_source.hip): what flockgpu_plan_feed does on the host -- testing validity, leaving rows out, rebasing
// Utf8 offsets -- for columns that already lie in HBM (flockgpu_plan_feed_columns, include/flockgpu_plan.h).  Three passes:
//   census         one launch over the validity bytes of every fed column that has them: NULLs per column, the rows that stay, and -- when a
//                  column whose NULL rows may be left out has validity -- the keep flags in the flag-tile geometry (scan.hpp); the same launch
//                  reads the first and last offset of every Utf8 column.  The answers land in pinned memory: one host wait.
//   rebased append a Utf8 column's offsets written behind the leaf's, already rebased onto its byte cursor: dst[i] = src[i] - src[0] + cursor
//   tail take      the rows of a row list, several fixed-width / validity columns per launch, written at a destination of ANY natural alignment
//                  (the leaf's tail is misaligned whenever the leaf holds an odd number of rows)
// Everything is queued on the ctx stream; only feed_census_wait waits.
#pragma once
#include "gather.hpp"

namespace flockgpu {

constexpr int kCensusCols = 64;   // validity columns per feed
constexpr int kCensusUtf8 = 32;   // Utf8 columns per feed

struct CensusArgs {
    const uint8_t *valid[kCensusCols];    // one byte per row, any alignment
    const int32_t *offsets[kCensusUtf8];  // rows + 1 entries
    uint64_t droppable = 0;               // bit c: a row whose valid[c] byte is 0 is left out
    int32_t n_valid = 0, n_utf8 = 0;
};
// What the census answers, in pinned memory (kPinnedPending until the kernel has written it).
struct CensusResult {
    const uint64_t *h = nullptr;   // [0, n_valid): NULLs per column; [kCensusCols]: rows kept; [kCensusCols + 1 + 2u], [.. + 2u + 1]: first / last offset of Utf8 column u
    int n_words = 0;
    int64_t nulls(int c) const { return (int64_t)h[c]; }
    int64_t kept() const { return (int64_t)h[kCensusCols]; }
    int64_t utf8_first(int u) const { return (int64_t)(int32_t)h[kCensusCols + 1 + 2 * u]; }
    int64_t utf8_last(int u) const { return (int64_t)(int32_t)h[kCensusCols + 2 + 2 * u]; }
    // set when droppable != 0: store_flags_and_counts' arrays over the kFlagTile-row tiles of [0, rows)
    uint32_t *flag_words = nullptr, *counts = nullptr;
    int32_t n_tiles = 0;
};
// Queues the census of `rows` (> 0) rows; `name` keys its arena / pinned buffers.  Nothing is launched when a.n_valid == 0 && a.n_utf8 == 0.
int feed_census_begin(flockgpu_ctx *ctx, const char *name, const CensusArgs &a, int64_t rows, CensusResult *out);
int feed_census_wait(flockgpu_ctx *ctx, const CensusResult &r);
// The census' keep flags -> the row numbers that stay, in order (`kept` of them; ctx-owned under `name`).  Queued, no wait.
int feed_census_rows(flockgpu_ctx *ctx, const char *name, const CensusResult &r, int64_t rows, int64_t kept, const int32_t **out_rows);

// dst[i] = src[i + 1] - src[0] + cursor for i in [0, n): the END offsets of n Utf8 values appended behind a column whose bytes end at `cursor`.
// dst and src need 4-byte alignment only.
int append_offsets_rebased(flockgpu_ctx *ctx, int32_t *dst, const int32_t *src, int64_t n, int32_t cursor);

// out[c][i] = src[c][rows[i]] for up to kGatherMulti columns of 1, 4 or 8 bytes per row in one launch; out[c] needs its element's alignment only.
struct TailTakeCols {
    const void *src[kGatherMulti];
    void *out[kGatherMulti];
    int32_t width[kGatherMulti];   // 1 | 4 | 8
    int32_t n = 0;
};
int take_to_tail(flockgpu_ctx *ctx, const TailTakeCols &cols, const int32_t *rows, int64_t n);

}  // namespace flockgpu
