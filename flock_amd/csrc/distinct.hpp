// COUNT(DISTINCT x) per group (HashAggregateExec's `distinct_count` aggregate): one streaming pass over (group id, argument) into a global
// open-addressing set of 8-byte slots, the slot form of relops.hpp key_codes under the conventions of hashtab.hpp.
//
// Assumptions (the fork's distinct_expressions.rs is not in the reference tree; upstream DataFusion ~6 DistinctCount, restated in DESIGN.md):
//   A-D1  the number of distinct non-NULL argument values among the group's rows, UInt64; NULL arguments are skipped; a group without a
//         valid value gives 0, never NULL.
//   A-D2  integers compare by value (Timestamp as its Int64), Utf8 bytewise; '' is a value, not NULL.
//   A-D7  the result depends on neither batching nor grid shape: a count is the number of claimed slots of its group, whoever claimed them.
//   (A-D3 .. A-D6 -- the key shapes, standing beside other aggregates, the Partial / Final modes, the order of the groups -- are the plan layer's:
//   plan_ir.hpp's header, plan.hip exec_aggregate)
#pragma once
#include "relops.hpp"

namespace flockgpu {

// counts[g] = distinct valid values of `arg` among the rows i with gid[i] == g, for g in [0, n_groups).  gid: int32 ids in [0, n_groups) (key_codes'),
// or null = every row in ONE group (n_groups must be 1).  arg: Int32 (read as 4 bytes) / Int64 / Timestamp / UInt64, or Utf8 -- which goes through
// utf8_codes first, the same kernel then runs over the codes; arg.valid is honoured, arg.all_null counts nothing.  `counts` (n_groups entries, caller-owned)
// is written entirely by the call.  Each valid row hashes (gid, value) to a slot {32-bit hash tag, first row}: the slot is LOADED first and the 64-bit
// compare-and-swap attempted on an empty slot only; the row whose claim succeeds adds 1 to counts[gid]; on a tag match the row compares
// (gid[first], value[first]) -- read from the input columns, which never change: a claimed slot is never seen half-filled -- with its own and is done
// when they are equal, else probes on.  A duplicate costs loads and no atomic; adds to `counts` are bounded by the distinct pairs.  Table and counts are
// cleared by a kernel.  The table is sized from the distinct pairs the call under this `name` saw last (two slots per row the first time: that always
// holds); probing is cut off as hashtab.hpp's, an overflow raises the error word and the pass is repeated ONCE with two slots per row.  Below 2^30 rows.
// One host wait (the error word).
int distinct_count_by_group(flockgpu_ctx *ctx, const char *name, const int32_t *gid, int64_t n_groups, const DevColumn &arg, int64_t rows, uint64_t *counts);

}  // namespace flockgpu
