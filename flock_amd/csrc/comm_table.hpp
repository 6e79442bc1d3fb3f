// The generic exchange behind flockgpu_plan_exchange_retain (include/flockgpu_comm.h): a whole table -- any number of Int32 / Int64 /
// UInt64 / Float64 / Timestamp and Utf8 columns, validity bytes included -- is hash-partitioned over the ranks of a communicator (or gathered
// on one of them), moved by the library's all-to-all and left on the device.  Defined in comm.hip next to exchange_relation, on the same
// transport (exchange_counts / all_to_all), with the same failure protocol; plan.hip is its one caller.
#pragma once
#include <string>
#include <vector>

#include "../../include/flockgpu_comm.h"
#include "relops.hpp"

namespace flockgpu {

struct XTableArgs {
    std::string name;                 // keys the arena buffers: the received columns must outlive the call ("plan<ptr>." names them after the plan)
    std::vector<DevColumn> cols;      // the table this rank contributes (type / is_ts / nullable are read even when rows == 0)
    int64_t rows = 0;                 // relation rows: with `sel`, the rows the selection keeps
    const int32_t *keys = nullptr;    // gather_rank < 0: one folded 32-bit key per relation row, 16-byte aligned (dest = (fmix32(key) * n_ranks) >> 32)
    const int32_t *sel = nullptr;     // may be null: relation row r is row sel[r] of `cols` (a filter's row list, composed with the send order)
    int gather_rank = -1;             // >= 0: every row goes to that rank, in input order (no keys, no sel)
    uint64_t fingerprint = 0;         // of the schema and the placement: compared across the ranks before anything moves
};
struct XTableResult {
    // n_ranks == 1: nothing was moved and nothing is returned -- the caller's table IS the result (one destination: send order is input order)
    bool passthrough = false;
    std::vector<DevColumn> cols;      // source-rank order, source order inside a source; `valid` set where ANY rank's column carried validity
    int64_t rows = 0;
};

// The communicator's phase timeline (flockgpu_comm_phase_*) around a call that starts outside comm.hip.
void exchange_phase_begin(flockgpu_comm *c);
void exchange_phase_mark(flockgpu_ctx *ctx, flockgpu_comm *c, const char *name);
void exchange_phase_finish(flockgpu_ctx *ctx, flockgpu_comm *c);
// Argument-level refusals that must come back BEFORE any collective: null / oversized / dead communicator.
int exchange_table_check(flockgpu_ctx *ctx, const flockgpu_comm *c, const char *what);
// entry_rc: this rank's status so far (its execute may have failed): the rank still takes part in the agreement, returns its own status, and
// every other rank returns FLOCKGPU_ERR_PEER.
int exchange_table(flockgpu_ctx *ctx, flockgpu_comm *c, int entry_rc, const XTableArgs &a, XTableResult *out);

}  // namespace flockgpu
