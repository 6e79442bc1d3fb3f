// What the two halves of the plan-level C ABI share: flock_amd/csrc/plan.hip (recognition, the executor, Arrow export) and
// flock_amd/csrc/plan_feed.hip (ingest: feeds, the pane ring, prefetch).  `struct flockgpu_plan` is a global type, so the types it is made of
// have a named namespace of their own -- one definition, whichever file looks.
#pragma once
#include <thread>

#include "../../include/flockgpu_plan.h"
#include "plan_ir.hpp"

namespace flockgpu {
namespace plan_detail {
#ifdef FLOCKGPU_EXPERIMENTAL
// (experimental builds: wall time per entry point, printed by flockgpu_plan_ring_close when FLOCKGPU_PLAN_TIMES is set)
struct ApiClock {
    const char *what;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    static std::map<std::string, std::pair<double, long>> &acc() {
        static std::map<std::string, std::pair<double, long>> m;
        return m;
    }
    explicit ApiClock(const char *w) : what(w) {}
    ~ApiClock() {
        auto &e = acc()[what];
        e.first += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        e.second += 1;
    }
    static void dump() {
        if (!flockgpu::exp_env("FLOCKGPU_PLAN_TIMES")) return;
        for (auto &kv : acc()) fprintf(stderr, "[plan times] %-28s %8ld calls %10.1f us/call\n", kv.first.c_str(), kv.second.second, kv.second.first / std::max(1L, kv.second.second));
        acc().clear();
    }
};
#define API_CLOCK(name) ApiClock api_clock_(name)
#define API_CLOCK2(var, name) ApiClock var(name)
#else
#define API_CLOCK(name) do {} while (0)
#define API_CLOCK2(var, name) do {} while (0)
#endif

// ------------------------------------------------------------------ tables
struct TCol {
    DevColumn c;
    bool present = false;
    // every value of this column is a value of the column at `subset_of` (it was taken from it by a filter, a join or as a GROUP BY's keys): when
    // that column is a leaf's, its cached minimum / maximum BOUND this one's -- enough to size the dense paths without a pass and a wait of its own
    const void *subset_of = nullptr;
};
struct Table {
    std::vector<TCol> cols;
    int64_t rows = 0;
};

struct DevBuf {  // a leaf column on the device, grown by feeds
    void *values = nullptr;  // fixed-width values or Utf8 bytes
    int32_t *offsets = nullptr;
    int64_t bytes = 0;
    // NULLs that may reach an output or an aggregate (round 4): one validity byte per row, materialised from the first batch that
    // holds such a NULL on; rows [0, valid_rows) are covered (the rest -- batches without NULLs -- is filled with 1 when the leaf is scanned)
    uint8_t *valid = nullptr;
    int64_t valid_rows = 0;
};
struct LeafData {
    std::vector<DevBuf> cols;
    int64_t rows = 0;
    int64_t dropped = 0;     // rows a feed left out because of NULLs
    bool borrowed = false;   // cols alias another plan's leaf (flockgpu_plan_feed_shared): nothing here is this leaf's to grow
    bool user_cols = false;  // ... or the caller's own columns (flockgpu_plan_feed_columns with FLOCKGPU_FEED_BORROW): the next feed copies them first
    // pane ring (flockgpu_plan_ring_open): rows -- and per Utf8 column, bytes -- of every pane whose rows this leaf still holds, oldest first
    std::vector<int64_t> pane_rows;
    std::vector<std::vector<int64_t>> pane_bytes;   // [pane][column]
};

enum Fused { kNone = 0, kQ2, kQ3, kQ5, kQ7, kQ8, kQ13, kPartialCount, kQ9, kQ4, kYsb };
struct FusedInfo {
    Fused kind = kNone;
    int leaf_a = -1, leaf_b = -1;     // the scans below
    std::vector<int> a_cols, b_cols;  // leaf columns handed to the fused entry point, in its argument order (-1: unused)
    std::vector<int> out_map;         // node output column -> fused output slot (-1: not produced)
    int64_t lit = 0;                  // q2 modulus / q3 category
    std::vector<std::string> strs;    // q3 state literals
};

constexpr int kStageLanes = 8;                     // at most this many host threads fill pinned chunks side by side (four do)
constexpr int kStageChunks = kStageLanes * 2;      // two chunks per lane: one is filled while the other is in flight
constexpr size_t kStageChunk = size_t(4) << 20;

}  // namespace plan_detail
}  // namespace flockgpu

struct flockgpu_plan {
    flockgpu_ctx *ctx = nullptr;
    flockgpu::ir::Plan ir;
    std::vector<flockgpu::plan_detail::LeafData> leaves;
    std::vector<flockgpu::plan_detail::FusedInfo> fused;  // by node id
    int query = 0;                 // NEXMark query number when the whole plan is one fused pipeline, else 0
    std::string description;
    bool generic_only = false;
    // pageable feeds go through a ring of pinned chunks: the host copies into chunk k + 1 while chunk k is in flight
    void *stage[flockgpu::plan_detail::kStageChunks] = {};
    hipEvent_t stage_done[flockgpu::plan_detail::kStageChunks] = {};
    int stage_next[flockgpu::plan_detail::kStageLanes] = {};
    struct CopyJob { void *dst; const void *src; size_t bytes; };
    std::vector<CopyJob> runs;   // transfers of the feed in progress, merged while they stay contiguous (h2d)
    int64_t fed_bytes = 0;
    bool device_fed = false;     // flockgpu_plan_feed_columns queued reads of the caller's device columns: reset waits for the stream before they may go
    flockgpu::plan_detail::Table retained;              // flockgpu_plan_execute_retain: the result, left on the device for the plans that consume it
    bool has_retained = false;
    // ---- device-side pane ring (flockgpu_plan.h): the last ring_ppw panes stay in HBM across executes
    int ring_ppw = 0;            // panes per window; 0: no ring, whole-window feeding
    int64_t ring_first = 0;      // id of the oldest pane held
    int ring_n = 0;              // panes held
    // q5 (COUNT GROUP BY auction -> MAX -> join): a pane is retained as its Partial aggregate state, the (auction, count) groups, in
    // `ring.q5a` / `ring.q5c` (pane after pane); the leaf holds only the newest pane's rows, until the next pane begins
    bool ring_q5 = false;
    std::vector<int64_t> ring_groups;   // groups per held pane (the newest pane's entry is valid when ring_newest_done)
    bool ring_newest_done = false;
    // flockgpu_plan_prefetch_pane: the NEXT pane's bytes on their way into side buffers (a stream of their own, host staging on threads of
    // their own) while the current window executes; flockgpu_plan_feed_pane(.., NULL, NULL, 0) for that pane appends them device to device
    struct Prefetch {
        bool active = false;
        int input = -1;
        int64_t pane = 0, rows = 0;
        std::vector<void *> dev;        // per leaf column: the side buffer (null: not prefetched); a Utf8 column's: its bytes
        std::vector<void *> dev_off;    // Utf8 columns: the pane's `rows` raw END offsets, batch by batch (rebased when the pane is appended)
        std::vector<int64_t> bytes;     // Utf8 columns: bytes in the side buffer
        struct Rebase { int col; int64_t row0, n; int64_t delta; };   // rows [row0, row0 + n) of column col: + delta turns a raw offset into a pane-relative one
        std::vector<Rebase> rebase;
        std::vector<std::thread> workers;
        std::vector<int> rc;
    } pre;
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_done = nullptr, append_done = nullptr;   // the pane's copies are queued / its side buffers have been read
    bool copy_done_set = false, append_done_set = false;
    int32_t *ring_auction = nullptr;
    uint32_t *ring_count = nullptr;
    // ---- flockgpu_plan_execute_async: the finished call's outputs, handed over by flockgpu_plan_wait
    bool async_pending = false;
    ArrowSchema async_schema{};
    std::vector<ArrowArray> async_batches;
    int async_n = 0;
    // ---- exact (min, max) of integer LEAF columns, computed when an operator first asks (the dense GROUP BY / join paths size their
    // direct-address tables from it) and kept while the leaf's contents stay what they were: every feed / reset / ring step drops them.
    // The reference's arch harness feeds once and executes ten times (flock-function/src/aws/arch/source.rs:25-65); a streaming host
    // pays one 4-byte-per-row pass per fed window.
    struct ColStat { int64_t rows, mn, mx; };
    std::map<const void *, ColStat> col_stats;
    // ---- common sub-plans: the signature of every Aggregate sub-tree that occurs more than once in the plan (q5's SQL names its
    // COUNT(*) GROUP BY auction subquery in both join inputs, q5_plan.fmt:6,13) and the scan leaves underneath it, by node id; an execute
    // runs such a sub-tree once per (signature, leaves its scans resolve to) and hands the table to its twins (Exec::memo)
    std::vector<std::string> twin_sig;               // empty: the node has no twin
    std::vector<std::vector<int>> twin_leaves;
    // ---- hash-placement guard: the scheme tag of the co-partitioned inputs fed since the last reset (-1: none fed yet)
    int scheme_state = -1;       // 0: untagged batches, 1: tagged with scheme_tag
    std::string scheme_tag;
};

namespace flockgpu {

inline std::string leaf_key(const flockgpu_plan *pl, int leaf, int col, const char *what) {
    char buf[96];
    snprintf(buf, sizeof buf, "plan%p.l%d.c%d.%s", (const void *)pl, leaf, col, what);
    return buf;
}
inline std::string node_key(const flockgpu_plan *pl, const ir::Node *n, const char *what, int i = 0) {
    char buf[96];
    snprintf(buf, sizeof buf, "plan%p.n%d.%s%d", (const void *)pl, n->id, what, i);
    return buf;
}

// ------------------------------------------------------------------ hash placement (flockgpu_plan.h)
constexpr const char *kPartitionScheme = "flockgpu/fmix32-mulhi/v1";
constexpr const char *kPartitionSchemeKey = "flockgpu.partition_scheme";
// value of `key` in an Arrow metadata blob; false when absent (or the blob is malformed)
inline bool find_metadata(const char *meta, const char *key, std::string *value) {
    if (!meta) return false;
    int32_t n = 0;
    std::memcpy(&n, meta, 4);
    const char *p = meta + 4;
    for (int32_t i = 0; i < n && n < 4096; ++i) {
        int32_t kl = 0, vl = 0;
        std::memcpy(&kl, p, 4);
        if (kl < 0 || kl > (1 << 20)) return false;
        const char *k = p + 4;
        std::memcpy(&vl, k + kl, 4);
        if (vl < 0 || vl > (1 << 20)) return false;
        const char *v = k + kl + 4;
        if ((size_t)kl == strlen(key) && !std::memcmp(k, key, (size_t)kl)) {
            value->assign(v, (size_t)vl);
            return true;
        }
        p = v + vl;
    }
    return false;
}

// ------------------------------------------------------------------ plan_feed.hip, called by the executor and by flockgpu_plan_destroy
int ring_q5_partial(flockgpu_plan *plan);   // (pane ring)
void prefetch_drop(flockgpu_plan *plan);

}  // namespace flockgpu
