// Generic relational operators over device columns, used by the plan interpreter (plan.hip) for every plan node that
// is not covered by one of the fused NEXMark pipelines: the STAGE plans either side of a `RepartitionExec Hash`
// (flock/src/distributed_plan/planner.rs:152-171, playground/.../nexmark/q{3,5,8}.dag; split rule
// flock/src/distributed_plan/stage.rs:269-367).  These run on the small, already filtered / aggregated relations of a
// stage, so they are written for generality (one lane per row, 64-bit normalised keys), not for the HBM roofline; the
// raw-row passes keep their fused kernels (q2 / q3 / q5 / q8 .hip).
//
// Semantics restated from upstream DataFusion ~6.x (not readable in the reference tree):
//   FilterExec keeps input order; HashAggregateExec groups compare by value (Utf8 bytewise); COUNT -> UInt64;
//   MAX ignores NULLs, an empty input gives NULL; inner HashJoinExec emits every matching pair, NULL keys never match.
#pragma once
#include <string>

#include "gather.hpp"
#include "sort.hpp"

namespace flockgpu {

enum class ColType : int32_t { I32 = 0, I64 = 1, U64 = 2, F64 = 3, UTF8 = 4 };
inline size_t col_width(ColType t) { return t == ColType::I32 ? 4 : 8; }

struct DevColumn {
    ColType type = ColType::I32;
    bool is_ts = false;     // Timestamp(Millisecond): Int64 storage, exported as "tsm:"
    bool nullable = false;  // schema flag only
    bool all_null = false;  // the single row of a global aggregate over no input (MAX -> NULL)
    // NULLs (round 4): one byte per row, 1 = valid; nullptr = every row valid (all NEXMark fields; the fused pipelines take only such
    // columns).  The slot of a NULL holds an unspecified value (a Utf8 NULL an empty or arbitrary range): every consumer looks here first.
    const uint8_t *valid = nullptr;
    const void *values = nullptr;      // fixed width values, or Utf8 bytes
    const int32_t *offsets = nullptr;  // Utf8 only, rows + 1 entries
    int64_t bytes = 0;                 // Utf8 only
};

enum class CmpOp : int32_t { EQ = 0, NE = 1, LT = 2, LE = 3, GT = 4, GE = 5 };

// ROW_NUMBER() of WindowAggExec over an input that arrives sorted by (PARTITION BY, ORDER BY): out[i] = 1 + i - (first row of the RUN of equal
// partition keys row i lies in); a run ends where any of the up to four key columns changes (NULL equals NULL; Float64 by its bits; Utf8 keys are
// refused).  No key column: the whole input is one run.  Launches only -- the caller's next wait covers it.
int row_number_runs(flockgpu_ctx *ctx, const char *name, const DevColumn *cols, int n_cols, int64_t rows, uint64_t *out);

// keys of an integer column as int64 (I32 sign-extended; I64 / U64 bit pattern): out[rows]
int widen_to_i64(flockgpu_ctx *ctx, const DevColumn &col, int64_t rows, int64_t *out);

// ---- take (a column's validity bytes are taken along)
int take_column(flockgpu_ctx *ctx, const char *name, const DevColumn &src, const int32_t *rows, int64_t n, DevColumn *out);
int gather_u8(flockgpu_ctx *ctx, const uint8_t *src, const int32_t *rows, int64_t n, uint8_t *out);
// keys[i] = sentinel where valid[i] == 0: NULL group keys form ONE group (DataFusion groups NULLs together), NULL hash-partition keys one place
int replace_invalid_i64(flockgpu_ctx *ctx, int64_t *keys, const uint8_t *valid, int64_t rows, int64_t sentinel);
// out[i] = keys[i] != sentinel (the validity of a group-key column that went through replace_invalid_i64); out[i] = count[i] != 0 (AVG over no valid value)
int valid_from_i64(flockgpu_ctx *ctx, const int64_t *keys, int64_t n, int64_t sentinel, uint8_t *out);

// ---- GROUP BY one integer key (as int64) with up to kMaxGroupAggs accumulators per group, all in one table (one pass over the rows).
// Outputs are ctx-owned, one entry per group (first_row: the smallest input row of the group).
// MAX_F64 / MIN_F64 order doubles through their order-preserving bit pattern (no NaN among the inputs: Arrow's min / max kernels
// skip NaN only against non-NaN values, a case the engine does not claim).
// Accumulators are 64-bit: COUNT (rows), SUM_INT (two's complement add of an integer column: Int32 sign-extended), MAX / MIN
// signed or unsigned, SUM_F64 (double add: exact -- hence order-free -- while every partial sum is an integer below 2^53, which
// is what AVG's partial sums of integer columns are).
enum class AggOp : int32_t { COUNT = 0, SUM_INT = 1, MAX_S = 2, MAX_U = 3, MIN_S = 4, MIN_U = 5, SUM_F64 = 6, MAX_F64 = 7, MIN_F64 = 8 };
constexpr int kMaxGroupAggs = 4;
struct AggSpec {
    AggOp op = AggOp::COUNT;
    const void *values = nullptr;  // null for COUNT
    ColType type = ColType::I64;   // storage type of `values`
    // validity of the argument (may be null): a NULL contributes to no accumulator -- COUNT(col) counts the valid rows, MIN / MAX / SUM
    // skip it (DataFusion's accumulators); a group none of whose values is valid comes out NULL (agg_valid)
    const uint8_t *valid = nullptr;
};
struct GroupResultN {
    int64_t n_groups = 0;
    int64_t *keys = nullptr;
    uint64_t *agg[kMaxGroupAggs] = {};  // 64-bit patterns: int64 / uint64 / double by AggOp
    uint8_t *agg_valid[kMaxGroupAggs] = {};  // per group: 1 when a valid value reached accumulator a; null when its spec carried no validity
    int32_t *first_row = nullptr;
    uint8_t *key_valid = nullptr;   // per group, when the call was given key validity: 0 for the NULL keys' group
};
// key_valid (may be null): rows whose key is NULL -- whatever their key bits -- form one group of their own
int group_by_key64_n(flockgpu_ctx *ctx, const char *name, const int64_t *keys, int64_t rows, const AggSpec *specs, int n_specs,
                     GroupResultN *out, const uint8_t *key_valid = nullptr);
// ---- dense integer keys: the perfect-hash variants of GROUP BY and JOIN.  Exact minimum / maximum of an integer column (signed order;
// unsigned for UInt64), through ONE synchronisation; `dense_range_ok`: the key range is affordable as a direct-address table for `rows` rows.
int column_minmax(flockgpu_ctx *ctx, const DevColumn &col, int64_t rows, int64_t *mn, int64_t *mx);
bool dense_range_ok(int64_t kmin, int64_t kmax, int64_t rows, bool uns);
// GROUP BY `key` (Int32 / Int64 / UInt64, no NULLs, every key inside [kmin, kmax]) with COUNT / SUM_INT / MIN / MAX accumulators over
// integer columns without NULLs: slot = key - kmin, tiles aggregated in LDS, groups come out in key order.  first_row / validity outputs
// are not produced (nothing on this path needs them).  A key outside [kmin, kmax] voids the call (FLOCKGPU_ERR_INVALID).
int group_by_dense(flockgpu_ctx *ctx, const char *name, const DevColumn &key, int64_t rows, int64_t kmin, int64_t kmax, const AggSpec *specs, int n_specs,
                   GroupResultN *out);
// ---- aggregate window functions of WindowAggExec (window.hip) over the default frame, RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW, on rows sorted
// by (PARTITION BY, ORDER BY): row i gets the aggregate of its partition's rows from the first through the last PEER of row i (equal ORDER BY values;
// without ORDER BY, the whole partition).  Keys compare as in row_number_runs (NULL equals NULL; Utf8 refused): keys[0, n_part) the PARTITION BY,
// keys[n_part, n_part + n_order) the ORDER BY, at most four each.  Accumulators are 64-bit as GROUP BY's (kMaxGroupAggs per pass of three launches;
// the keys are compared in the first pass only): COUNT counts valid arguments (`valid` null: every row), SUM_INT wraps, MIN / MAX signed, unsigned or
// Float64; AVG = double(int64 SUM) / double(COUNT).  NULL arguments are skipped; out_valid[i] = 0 while no valid value is in row i's frame (AVG: no
// value; COUNT writes none).  `out_type` I32 narrows the result.  Below 2^31 rows; launches only.
struct WinAgg {
    AggOp op = AggOp::COUNT;        // COUNT | SUM_INT | MAX_S | MAX_U | MIN_S | MIN_U | MAX_F64 | MIN_F64 (ignored for AVG)
    bool avg = false;
    const void *values = nullptr;   // the argument (null: COUNT(*))
    ColType type = ColType::I64;    // its storage type
    const uint8_t *valid = nullptr;
    void *out = nullptr;            // rows values of out_type (Int32: 4 bytes, else 8)
    ColType out_type = ColType::I64;
    uint8_t *out_valid = nullptr;   // may be null
};
int window_aggregates(flockgpu_ctx *ctx, const char *name, const DevColumn *keys, int n_part, int n_order, int64_t rows, const WinAgg *aggs, int n_aggs);

// ---- Utf8 keys (YSB joins and groups on UUID strings, flock/src/distributed_plan/planner.rs:298-346)
// out[i] = 64-bit hash of row i's bytes: equal strings -> equal keys (enough for a hash repartition; NOT an equality test)
int hash_utf8_i64(flockgpu_ctx *ctx, const DevColumn &col, int64_t rows, int64_t *out);
// Exact dictionary codes: codes[i] = row number of the first-inserted row of `build` with the same bytes (a hash table of row
// numbers with a full byte compare on every hit).  probe_codes[j] = the code of the equal `build` string, or -(j + 2) when
// `build` does not contain it (negative codes are pairwise different and match nothing).  Either output may be null.
int utf8_codes(flockgpu_ctx *ctx, const char *name, const DevColumn &build, int64_t n_build, int64_t *build_codes, const DevColumn *probe,
               int64_t n_probe, int64_t *probe_codes);
// ---- composite keys: a tuple of 1..kMaxKeyCols columns (Int32 / Int64 / Timestamp / UInt64 / Utf8; NULLs allowed) -> one dense id per row.
// Integers compare by value after widening to 64 bits (an Int32 column meets an Int64 one; UInt64 meets only UInt64 -- the caller's check),
// Utf8 bytewise, NULL equals NULL within a column.  gid[i] in [0, *n_groups), numbered in order of first appearance; *first_rows (ctx-owned,
// ascending) = the first row of every group.  A probe side (may be absent): probe_gid[j] = the id of the equal build tuple, or -1 when the
// build side does not hold it or any of the probe's key columns is NULL there.  Global open-addressing table of 8-byte slots (32-bit hash
// tag, 32-bit first row: an atomic minimum keeps the first row), full tuple compare only where the tags agree.  One host wait.  Build side below
// 2^30 rows (the table's slot numbers travel as int32), probe side below 2^31.
constexpr int kMaxKeyCols = 8;
int key_codes(flockgpu_ctx *ctx, const char *name, const DevColumn *build_cols, int n_cols, int64_t rows, int32_t *gid, int64_t *n_groups,
              int32_t **first_rows, const DevColumn *probe_cols, int64_t probe_rows, int32_t *probe_gid);
// dst[ids[i]] = src[i] for i in [0, n): the groups of a hashed GROUP BY over dense ids put back in id order (8-byte or 1-byte elements)
int scatter_by_id_u64(flockgpu_ctx *ctx, const int64_t *ids, int64_t n, const uint64_t *src, uint64_t *dst);
int scatter_by_id_u8(flockgpu_ctx *ctx, const int64_t *ids, int64_t n, const uint8_t *src, uint8_t *dst);
// (a, b) Int32 pairs <-> one 64-bit key: key = (int64(a) << 32) | uint32(b)
int pack_i32_pair(flockgpu_ctx *ctx, const int32_t *a, const int32_t *b, int64_t n, int64_t *out);
int unpack_i32_pair(flockgpu_ctx *ctx, const int64_t *keys, int64_t n, int32_t *a, int32_t *b);
// out[i] = (double)in[i]
int i64_to_f64(flockgpu_ctx *ctx, const int64_t *in, int64_t n, double *out);
// out[i] = sum[i] / (double)count[i]   (AVG's finish: one IEEE division, as DataFusion's AvgAccumulator::evaluate)
int avg_finish(flockgpu_ctx *ctx, const double *sum, const uint64_t *count, int64_t n, double *out);
// GROUP BY (int32 key, Utf8 value) without aggregates = DISTINCT over both columns: the first row of every distinct pair,
// ascending.
int distinct_i32_utf8(flockgpu_ctx *ctx, const char *name, const int32_t *key, const flockgpu_utf8 &text, int64_t rows,
                      int32_t **out_rows, int64_t *n_out);
// MAX of an integer column (signed, or unsigned for UInt64) as its 64-bit pattern, on the host; *any = 0 when there is no (valid) row.
int reduce_max(flockgpu_ctx *ctx, const DevColumn &col, int64_t rows, int64_t *out, int *any);

// ---- inner equi-join on one 64-bit key: every (left_row, right_row) pair with equal keys, ordered by right row
// (the probe side); the left rows of one right row come in the build chain's order, which is NOT defined (concurrent push-front
// inserts) -- callers compare multisets, as the reference does (test_util.rs:61-90).  Builds on the left (DataFusion's build side).
// More than 2^31 - 1 pairs: FLOCKGPU_ERR_UNSUPPORTED, decided from a 64-bit total before anything is emitted.
int join_key64(flockgpu_ctx *ctx, const char *name, const int64_t *left, int64_t n_left, const int64_t *right, int64_t n_right,
               int32_t **left_rows, int32_t **right_rows, int64_t *n_pairs);
// The table path of join_key64 with the keys read in their columns' own types (Int32 / Int64 / UInt64 of one signedness, no NULLs): 16-byte
// slots (key, claiming row, chain head), unique build keys probed as a filter in the flag-tile geometry.  Builds on the smaller side.
int join_hashed(flockgpu_ctx *ctx, const char *name, const DevColumn &left, int64_t n_left, const DevColumn &right, int64_t n_right,
                int32_t **left_rows, int32_t **right_rows, int64_t *n_pairs);
// join_key64 answers this pair of sizes with ONE workgroup and one launch (table, heads and chain links in LDS): no statistics, no dense path needed
bool join_is_tiny(int64_t n_left, int64_t n_right);

// The same join when the BUILD side's keys are dense (every key of `left` inside [kmin, kmax], range affordable: dense_range_ok): chain heads
// addressed by key - kmin, keys read in their columns' own types.  Pairs ordered by right row, as join_key64's.
int join_dense(flockgpu_ctx *ctx, const char *name, const DevColumn &left, int64_t n_left, int64_t kmin, int64_t kmax, const DevColumn &right, int64_t n_right,
               int32_t **left_rows, int32_t **right_rows, int64_t *n_pairs);

// ---- semi / anti join (HashJoinExec join_type Semi / Anti): the rows of `left` -- ascending, each at most once -- for which at least one (Semi) or
// no (Anti) row of `right` holds an equal key.  Assumptions (the fork's hash_join.rs is not in the reference tree; upstream DataFusion ~5/6, where
// JoinType::{Semi, Anti} exist on HashJoinExec):
//   A-S1  Semi: left rows with at least one right row equal in every key pair; Anti: left rows with none.
//   A-S2  The output schema is the left input's; the right side contributes no column.
//   A-S3  A left row appears at most once, however many right rows match it; left rows with equal keys are kept or dropped each on its own.
//   A-S4  A NULL in any key column equals nothing: a NULL-keyed right row is never a match; a NULL-keyed left row is dropped by Semi and KEPT by
//         Anti; with an empty right side Semi returns nothing and Anti every left row.
//   A-S5  Rows come out in left input order (upstream emits from the build side's visited bitmap in index order): a stable filter of the left side.
//   A-S6  Both modes (Partitioned, CollectLeft) are taken; which side carries the table is unobservable.
// The right side is a SET -- a bitmap over [kmin, kmax] when `dense` (every right key inside it, dense_range_ok for n_right rows), else a hashed
// table of 8-byte key slots -- and the left side is probed as a filter in the flag-tile geometry, then count -> scan -> emit.  Integer keys of one
// signedness read in their columns' own types; `left.valid` is honoured (a NULL left key matches nothing), `right` holds no NULLs (the caller
// drops them).  A left key outside [kmin, kmax] matches nothing.  *rows: ctx-owned.  One host wait.
int semi_rows(flockgpu_ctx *ctx, const char *name, const DevColumn &left, int64_t n_left, const DevColumn &right, int64_t n_right, bool dense, int64_t kmin,
              int64_t kmax, bool anti, int32_t **rows, int64_t *n_out);
// semi_rows answers this pair of sizes with ONE workgroup and one launch (the right keys as a set in LDS): no statistics, no bitmap needed
bool semi_is_tiny(int64_t n_left, int64_t n_right);
// The same from per-left-row ids that already say "absent" with a negative value (utf8_codes' probe codes: int64; key_codes' probe ids: int32, -1
// where a key column of the left row is NULL).
int semi_rows_from_ids(flockgpu_ctx *ctx, const char *name, const void *ids, bool ids64, int64_t n_left, bool anti, int32_t **rows, int64_t *n_out);

// ---- hash partition: rows grouped by destination (input order kept): dest = (fmix32(fold(key)) * n) >> 32, the
// mix of flockgpu_partition_by_key.  part_offsets: host, n_parts + 1.
int partition_rows_key64(flockgpu_ctx *ctx, const char *name, const int64_t *keys, int64_t rows, int32_t n_parts, int32_t **out_rows,
                         std::vector<int64_t> *part_offsets);
// the fold alone: out[i] = low ^ high word of keys[i], the 32-bit key the partition pass mixes (the table exchange partitions by it, comm_table.hpp)
int fold_keys_i32(flockgpu_ctx *ctx, const int64_t *keys, int64_t rows, int32_t *out);

// ---- ORDER BY (SortExec; the reference's boundary goldens end in it, flock/src/runtime/context.rs:471,549, and the stage splitter
// cuts at it, flock/src/distributed_plan/stage.rs:337): the permutation of [0, rows) that orders the rows by `keys`, first key most
// significant, ties in input order (stable).  LSD over the keys: every key becomes an order-preserving unsigned 64-bit value in the
// current order (Int32 / Int64 / Timestamp: sign bit flipped; UInt64: as is; Float64: A-FO1 below -- the order key of the value after
// f64_canonical_bits (orderkey.hpp), so the two zeros tie and every NaN ties above +inf; Utf8: bytewise
// lexicographic -- the length as the least significant sub-key, then 8-byte big-endian chunks from the last to the first;
// descending: complemented), its range is read back (one wait per sub-key; a constant sub-key costs no pass) and the stable radix
// passes of sort.hpp run over the bits the range needs.  *out_rows: ctx-owned, `rows` entries.  Columns hold no NULLs
// (`nulls_first` has nothing to place); an all-NULL column ties every row.
//
// How Float64 values order and compare.  ASSUMPTIONS: the arrow fork the reference builds against is not at hand; the rule is arrow-rs' of that
// time (`cmp_nans_last` over `partial_cmp`), pinned by tests/float_order_ref.py.
//   A-FO1  ORDER BY.  Ascending: -inf < ... < -5e-324 < {-0.0, +0.0} < 5e-324 < ... < +inf < {every NaN}.  The two zeros tie; all NaNs tie,
//          whatever their sign and payload; ties keep input order (the sort is stable).  DESC is the exact reverse on values (NaNs first among
//          the non-NULL rows), ties still in input order.  NULLs: `nulls_first` decides, DESC does not move them.
//   A-FO2  WindowAggExec and ROW_NUMBER.  Two Float64 key values lie in one partition, or one peer group, exactly when A-FO1 ties them.
//   A-FO3  Filters and computed comparisons are IEEE: a comparison with a NaN operand is FALSE, except `<>`, which is TRUE; -0.0 = +0.0;
//          subnormals are numbers like any other, nothing is flushed.
//   A-FO4  MIN / MAX compare order keys (orderkey.hpp f64_order_key): -0.0 lies below +0.0, and "no NaN among the inputs" stays the precondition.
//   A-FO5  Values that pass through a take, a union, a cross join or an exchange keep their bits, NaN payloads included.
struct SortKey {
    DevColumn col;
    bool descending = false;
    bool nulls_first = false;   // where the rows whose col.valid is 0 go (SortOptions of the plan; DESC does not move them)
};
// sorted_i32 (may be null): set to the first key's column IN ITS SORTED ORDER when the sort made one on the way (one ascending Int32 key without
// NULLs: the radix sort carries the column itself), else to null -- the caller's take of that column is then a pointer.
int sort_rows(flockgpu_ctx *ctx, const char *name, const SortKey *keys, int n_keys, int64_t rows, int32_t **out_rows, const int32_t **sorted_i32 = nullptr);
// keys[order[i]] is non-decreasing in i (sort_rows' output): starts = the positions i where a new key begins (ascending; device), *n_keys of them.
// One host wait.
int key_run_starts(flockgpu_ctx *ctx, const char *name, const int64_t *keys, const int32_t *order, int64_t rows, int32_t **starts, int64_t *n_keys);

// u32 -> u64 (COUNT partial states are UInt64 in the reference's schemas)
int widen_u32_to_u64(flockgpu_ctx *ctx, const uint32_t *in, int64_t n, uint64_t *out);
// int64 -> int32 (group keys go back to the type of their column)
int narrow_i64_to_i32(flockgpu_ctx *ctx, const int64_t *in, int64_t n, int32_t *out);
// data[i] += delta for i in [0, n): Utf8 offsets of an appended batch rebased onto the column's byte cursor
int add_i32(flockgpu_ctx *ctx, int32_t *data, int64_t n, int32_t delta);

}  // namespace flockgpu
