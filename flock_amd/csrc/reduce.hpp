// Ungrouped aggregates (HashAggregateExec without GROUP BY): every accumulator of one node in ONE streaming pass over the rows, optionally under the
// flag words a predicate pass left (pred.hpp pred_to_flags), then a one-workgroup fold that writes the node's single result row on the device.
// Nothing comes back to the host: the row count is 1 by construction.
//
// A node is restated as
//   columns : the DISTINCT argument columns (Int32 / Int64 / UInt64 / Timestamp / Float64), each streamed once, with its validity bytes if it has them;
//   slots   : one 64-bit register accumulator per lane each -- a wrapping integer sum, an exact Float64 sum (AVG's sum states: integers below 2^53),
//             or an unsigned maximum of an order key (signed: bits ^ sign; Float64: relops' f64_order_key; a minimum is the maximum of the complement);
//   counts  : per column, the rows that reached its slots (valid, and selected by the flag words);
//   outputs : the result row's columns, finished by the fold from slots and counts (AVG's division, the Partial state layout, NULL over no value).
// Every combination is associative and commutative on the bits, partials are combined by plain stores into a slab and a second launch: the result
// does not depend on the grid or on the order workgroups finish in.
#pragma once
#include "relops.hpp"

namespace flockgpu {

constexpr int kReduceMaxCols = 8;
constexpr int kReduceMaxSlots = 8;
constexpr int kReduceMaxOuts = 16;
// Workgroups per CU of the streaming pass; a relation of more tiles than the grid has workgroups is walked tile b, b + G, ...  (One tile per
// workgroup was tried: GA-price's pass 0.139 ms against 0.114 ms, and a slab of one row per tile costs the one-workgroup fold 0.03 ms more.)
constexpr int kReduceBlocksPerCu = 8;

enum class ReduceKind : int32_t { SumInt = 0, UMax = 1, SumF64 = 2 };
struct ReduceCol {
    const void *values = nullptr;
    const uint8_t *valid = nullptr;
    int32_t type = 0;   // ColType
    int32_t pad = 0;
};
struct ReduceSlot {
    int32_t kind = 0;    // ReduceKind
    int32_t col = 0;
    uint64_t flip = 0;   // UMax: key = bits ^ flip (sign bit for signed / Float64 order, all ones more for a minimum)
    int32_t f64 = 0;     // UMax over Float64: the magnitude bits of a negative value are complemented too
    int32_t inv = 0;     // UMax: a minimum
};
enum class ReduceOutKind : int32_t {
    Rows = 0,        // COUNT(*): the rows selected
    ColCount = 1,    // COUNT(col), AVG's count state: count of `col`
    Value = 2,       // SUM / MIN / MAX: slot a decoded; NULL while count of `col` is 0
    ValueAlways = 3, // Final COUNT: slot a, never NULL
    SumAsF64 = 4,    // AVG's sum state: (double) of the integer sum in slot a (b: the column is unsigned)
    AvgFinal = 5,    // Final AVG: Float64 sum of slot b / (double) integer sum of slot a; NULL while that is 0
    AvgOnePass = 6,  // AVG finished in one pass (a node with a distinct count): (double) of the integer sum in slot a (b: unsigned) / (double) count of `col`;
                     // NULL while the count is 0 -- the division Final makes of the one (count, sum) state row
};
struct ReduceOut {
    int32_t kind = 0;
    int32_t col = 0;
    int32_t a = 0, b = 0;
};
struct ReduceProgram {
    ReduceCol cols[kReduceMaxCols];
    ReduceSlot slots[kReduceMaxSlots];
    ReduceOut outs[kReduceMaxOuts];
    int32_t n_cols = 0, n_slots = 0, n_outs = 0, pad = 0;
};

// Runs `prog` over `rows` rows.  flag_words / wave_counts (both or neither; n_flag_tiles tiles): only flagged rows count.  out_values[o] (64-bit; an
// Int32 result sits in the low word) and out_valid[o] get output o.  Launches only: no wait, nothing read back.
int reduce_global(flockgpu_ctx *ctx, const char *name, const ReduceProgram &prog, int64_t rows, const uint32_t *flag_words, const uint32_t *wave_counts,
                  int32_t n_flag_tiles, uint64_t *out_values, uint8_t *out_valid);

}  // namespace flockgpu
