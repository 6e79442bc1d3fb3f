// GROUP BY with five to sixteen accumulators per node (NEXMark q17's auction statistics carry nine): ONE streaming pass over dense group ids that
// loads every distinct argument column and every distinct validity column once per row and updates [cell][group] 64-bit cells -- the grouped twin of
// the ungrouped pass (reduce.hpp).  The tables of relops.hpp keep their four accumulators (kMaxGroupAggs sizes their register arrays); a node with
// more gets its ids from key_codes whatever its key shape and comes here, so its groups come out in order of first appearance.
//
// Semantics are GROUP BY's (relops.hpp): COUNT counts the rows whose argument is valid (no validity: every row), SUM_INT wraps in 64 bits (Int32
// sign-extended), MIN / MAX are signed, unsigned or Float64 (through orderkey.hpp), SUM_F64 adds doubles -- Final mode's sum of AVG states: exact, hence
// order-free, while every partial sum is an integer below 2^53, which the Partial's sums of integer columns are; beyond that the order of the adds,
// which atomics do not fix, shows in the last bit, as it does in the table of relops.hip.  NULL arguments reach no cell.
//
// Validity is kept per distinct validity column, not per accumulator: one "valid rows" cell per (validity column, group).  It IS the COUNT of every
// argument that carries that validity, and an accumulator's NULL-ness is read from it at the finish.
#pragma once
#include "relops.hpp"

namespace flockgpu {

constexpr int kMaxWideAggs = 16;   // accumulators of one node (AVG takes two)
constexpr int kMaxWideCols = 16;   // distinct (values, validity) argument columns of one node: every accumulator may read a column of its own (a Final's state columns do)

// One result column of an aggregate node, described from the node's accumulators.  The lowering of plan.hip (lower_aggregates) writes one per column
// behind the keys, and all three back-ends read the same list: this pass finishes its columns on the device, the tables of relops.hpp finish them
// with helper launches, the ungrouped pass (reduce.hpp) restates them as its outputs.  Int32 results are narrowed where `type` says so.
enum class WideOutKind : int32_t {
    Value = 0,          // the accumulator: a count, a sum, a minimum or maximum (Float64 ones back from their order keys)
    SumAsF64 = 1,       // (double) the integer sum: the sum state of a Partial's AVG
    AvgInt = 2,         // (double) integer sum acc2 / (double) count acc: AVG in one pass
    AvgF64 = 3,         // Float64 sum acc2 / (double) count acc: AVG in Final mode
    DistinctCount = 4,  // no accumulator: a table of its own over the group ids (distinct.hpp); `acc` is the aggregate's place in the node.  Never handed to this pass.
};
struct WideOut {
    WideOutKind kind = WideOutKind::Value;
    int acc = 0, acc2 = -1;
    ColType type = ColType::I64;   // of the result column (I32: narrowed)
    // 0: no validity column is written; 1: valid while accumulator `acc` saw a valid value (MIN / MAX / SUM over nothing but NULLs is NULL) -- none is
    // written when its argument carries no validity; 2: valid while count `acc` is not 0 (AVG)
    int validity = 0;
};
struct WideGroupResult {
    void *col[kMaxWideAggs] = {};        // n_groups values each, ctx-owned
    uint8_t *valid[kMaxWideAggs] = {};   // null: every group valid
};
// LDS bins per tile for a node of n_specs accumulators (a tile whose ids span more goes to the global cells directly)
int wide_group_bins(int n_specs);
// gid[i] in [0, n_groups): one Int32 per row (key_codes').  Launches only: an id outside [0, n_groups) reaches no cell.
int group_by_ids_wide(flockgpu_ctx *ctx, const char *name, const int32_t *gid, int64_t rows, int64_t n_groups, const AggSpec *specs, int n_specs,
                      const WideOut *outs, int n_outs, WideGroupResult *out);

}  // namespace flockgpu
