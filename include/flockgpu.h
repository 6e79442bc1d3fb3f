/* flockgpu.h -- C ABI of libflockgpu, the MI355X (gfx950) execution kernel for Flock's
 * per-batch DataFusion hot path (filter, projection, hash-join, hash-aggregate over NEXMark
 * RecordBatches).  Plain C, plain pointers and sizes: this is exactly what a Rust
 * `extern "C"` block in flock/src/runtime would bind (INTEGRATION.md shows the stub).
 *
 * Every entry point returns an int status (FLOCKGPU_OK = 0); nothing throws or aborts across
 * the ABI; `flockgpu_last_error(ctx)` returns the message of the last failure on that ctx.
 * (The reference stringifies DataFusion errors into FlockError::Execution and then
 * unwraps them, flock/src/runtime/context.rs:181,189 -- i.e. an operator error kills the
 * Lambda; here it is a status code the host can turn into FlockError::Execution.)
 *
 * Threading: a ctx (stream + device arena) is used by one thread at a time; different ctxs
 * may be used concurrently from arbitrary threads (the reference runs each plan on its own
 * tokio task, context.rs:178).  No global mutable state.
 *
 * Memory: all column pointers in the `*_cols` views are DEVICE pointers (HBM) laid out
 * exactly like the corresponding Arrow buffers (values; int32 offsets + bytes for Utf8;
 * all NEXMark fields are non-nullable, event.rs:130-149,220-245,336-352).  They are
 * BORROWED for the duration of the call and never written (the reference asserts inputs
 * survive execution, datasource/nexmark/queries/q5.rs:127-131).  Result buffers are owned
 * by the ctx arena and stay valid until the next call of the same query on that ctx or
 * flockgpu_ctx_destroy.
 */
#ifndef FLOCKGPU_H
#define FLOCKGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLOCKGPU_ABI_VERSION 1

enum {
    FLOCKGPU_OK = 0,
    FLOCKGPU_ERR_INVALID = 1,     /* bad argument                                            */
    FLOCKGPU_ERR_HIP = 2,         /* a HIP runtime call failed (message has the hipError)     */
    FLOCKGPU_ERR_OOM = 3,         /* device arena allocation failed                           */
    FLOCKGPU_ERR_UNSUPPORTED = 4, /* plan shape / size outside what the kernels implement     */
    FLOCKGPU_ERR_CAPACITY = 5,    /* hash table overflow after the retry budget               */
    FLOCKGPU_ERR_PLAN = 6,        /* plan JSON could not be parsed / matched                  */
    FLOCKGPU_ERR_PEER = 7         /* exchange: another rank of the communicator failed (flockgpu_comm.h); this rank's inputs are fine */
};

typedef struct flockgpu_ctx flockgpu_ctx;

/* ---- context ------------------------------------------------------------------------------- */
/* `hip_stream` may be NULL (the ctx creates its own stream, ordered against the legacy default
 * stream like any blocking HIP stream) or an existing hipStream_t the caller launches on. */
int flockgpu_ctx_create(int device, void *hip_stream, flockgpu_ctx **out);
void flockgpu_ctx_destroy(flockgpu_ctx *ctx);
const char *flockgpu_last_error(const flockgpu_ctx *ctx);
int flockgpu_ctx_synchronize(flockgpu_ctx *ctx);
int flockgpu_abi_version(void);

/* ---- plain memory helpers (hosts without their own HIP binding) --------------------------------- */
enum { FLOCKGPU_H2D = 1, FLOCKGPU_D2H = 2, FLOCKGPU_D2D = 3 };
int flockgpu_malloc(flockgpu_ctx *ctx, size_t bytes, void **out_device_ptr);
int flockgpu_free(flockgpu_ctx *ctx, void *device_ptr);
/* Copies on the ctx stream and waits for completion. */
int flockgpu_memcpy(flockgpu_ctx *ctx, void *dst, const void *src, size_t bytes, int kind);
/* Testing aid: device memory that ENDS where mapped address space ends (`bytes` rounded up to 16, placed at the tail of its own
 * physical allocation; the address granule behind it is reserved and left unmapped).  A kernel that touches memory past the end of a
 * column placed there faults -- with ordinary allocations it reads whatever lies next to it and nobody notices.  Freed with
 * flockgpu_free_guarded (or with the ctx): the physical memory goes back, the address range stays reserved for the life of the
 * process, so that no guarded address is ever handed out twice. */
int flockgpu_malloc_guarded(flockgpu_ctx *ctx, size_t bytes, void **out_device_ptr);
int flockgpu_free_guarded(flockgpu_ctx *ctx, void *device_ptr);

/* Per-kernel HIP-event timing (bench.py's roofline leg).  When enabled, every kernel launch of
 * the ctx is bracketed by hipEvents on the ctx stream; totals are read back per kernel name. */
int flockgpu_profile_enable(flockgpu_ctx *ctx, int on);
/* Restricts the bracketing to launches of one kernel (NULL: every kernel again), or of any of several: "a|b" -- the kernels a call
 * chooses between for one step (q3's probe runs `q3_probe_flag_small_kernel` while all its tiles are resident at once, else
 * `q3_probe_flag_kernel`).  Two event records per launch are markers on the stream: bracketing all ~20 launches of a small-batch
 * query costs as much as its kernels. */
int flockgpu_profile_only(flockgpu_ctx *ctx, const char *kernel_name);
int flockgpu_profile_reset(flockgpu_ctx *ctx);
/* Fills up to `cap` entries; returns the number of distinct kernels seen in *n. */
typedef struct {
    char name[48];
    uint64_t launches;
    double total_ms;
} flockgpu_kernel_stat;
int flockgpu_profile_read(flockgpu_ctx *ctx, flockgpu_kernel_stat *out, int cap, int *n);
/* The per-launch durations behind one kernel's total, in launch order (the first 4096 since the last reset): *n = how many
   exist, out_ms receives min(*n, cap) of them.  A HIP-event pair also spans the host's gap between recording the start event and
   enqueueing the kernel when the stream is idle, so for 10-microsecond kernels one preempted launch can double a 20-launch mean;
   the spread (bench.py reports min / median / max beside the mean) shows it. */
int flockgpu_profile_samples(flockgpu_ctx *ctx, const char *kernel_name, float *out_ms, int cap, int *n);

/* ---- column views (device pointers, Arrow buffer layout) -------------------------------------- */
typedef struct { /* Bid::schema, event.rs:336-352 */
    const int32_t *auction, *bidder, *price;
    const int64_t *b_date_time;
    int64_t rows;
} flockgpu_bid_cols;

typedef struct { /* Auction::schema projection used by q3/q8 (q3_plan.fmt:4, q8_plan.fmt:10) */
    const int32_t *a_id, *seller, *category;
    int64_t rows;
} flockgpu_auction_cols;

typedef struct { /* Arrow Utf8: offsets has rows+1 entries */
    const int32_t *offsets;
    const uint8_t *data;
} flockgpu_utf8;

typedef struct { /* Person::schema projection used by q3/q8 (q3_plan.fmt:6, q8_plan.fmt:6) */
    const int32_t *p_id;
    flockgpu_utf8 name, city, state;
    int64_t rows;
} flockgpu_person_cols;

/* A window schedule over one relation: `n_panes + 1` row offsets (HOST pointer) delimit
 * consecutive, disjoint panes of rows; window w covers panes [win_pane_lo[w], win_pane_hi[w]).
 *   ElementWise  (window/elementwise.rs:46)   : pane = 1-s epoch, window = 1 pane
 *   Tumbling(s)  (window/tumbling.rs:55-57)   : pane = s epochs,  window = 1 pane
 *   Hopping(w,h) (window/hopping.rs:54-57)    : pane = gcd(w,h) epochs, window = w/gcd panes, stride h/gcd
 * One call executes every window of the schedule = the reference's per-window loop of
 * `actor::collect` (flock-function/src/aws/actor.rs:54-79) batched into a few launches. */
typedef struct {
    const int64_t *pane_row_offsets; /* host, n_panes + 1, non-decreasing */
    int32_t n_panes;
    const int32_t *win_pane_lo; /* host, n_windows */
    const int32_t *win_pane_hi; /* host, n_windows */
    int32_t n_windows;
} flockgpu_windows;

/* ---- q1: ProjectionExec [auction, bidder, 0.908 * CAST(price AS Float64) AS price, b_date_time]
 * (planner.rs:90, q1_plan.fmt:1).  Pass-through columns are zero-copy in the reference (Arc
 * clones); the kernel materialises only the computed Float64 column.  `factor` = the literal. */
int flockgpu_q1_project(flockgpu_ctx *ctx, const flockgpu_bid_cols *bid, double factor,
                        double *out_price /* device, bid->rows */);

/* ---- q2: FilterExec CAST(auction AS Int64) % modulus = 0 -> CoalesceBatches -> Projection
 * [auction, price] (planner.rs:120-124, q2_plan.fmt:1-3).  Stable: input row order is kept.
 * out_*: device buffers in the ctx arena; win_out_offsets: HOST array of n_windows + 1 row
 * offsets into out_* (arena-owned).  Requires single-pane windows (ElementWise). */
typedef struct {
    const int32_t *auction, *price;   /* device */
    const int64_t *win_out_offsets;   /* host, n_windows + 1 */
    int64_t rows;
} flockgpu_q2_result;
int flockgpu_q2_filter(flockgpu_ctx *ctx, const flockgpu_bid_cols *bid, const flockgpu_windows *win,
                       int64_t modulus, flockgpu_q2_result *out);

/* ---- q3: Filter(category = lit) on auction, Filter(state = l0 OR state = l1 OR ...) on person,
 * HashJoinExec(Inner, seller = p_id), Projection [name, city, state, a_id]
 * (planner.rs:152-171, q3_plan.fmt:1-6).  `auction_win` / `person_win` describe the same
 * n_windows windows over the two relations.  Output rows are grouped by window, ordered by
 * auction row inside a window (row order across partitions is not a contract in the reference:
 * results compare as sorted multisets, test_util.rs:61-90). */
typedef struct {
    flockgpu_utf8 name, city, state;  /* device */
    const int32_t *a_id;              /* device */
    const int32_t *auction_row, *person_row; /* device: matching input row pairs */
    const int64_t *win_out_offsets;   /* host, n_windows + 1 */
    int64_t rows;
    int64_t name_bytes, city_bytes, state_bytes;
} flockgpu_q3_result;
int flockgpu_q3_join(flockgpu_ctx *ctx, const flockgpu_auction_cols *auction, const flockgpu_windows *auction_win,
                     const flockgpu_person_cols *person, const flockgpu_windows *person_win,
                     int64_t category_lit, const char *const *state_lits, int n_state_lits,
                     flockgpu_q3_result *out);

/* ---- q5: COUNT(*) GROUP BY auction; MAX(num); rows with num = maxn, ties kept
 * (q5.sql, q5_plan.fmt:1-13, q5.dag).  Hopping windows share panes: every bid is read once.
 * Output: per window, (auction Int32, num UInt64) rows sorted by auction.
 * The call returns with its results complete and may leave one clean-up kernel queued on the ctx stream (it zeroes the counters the
 * call used, so that the next call does not have to): work the caller queues on the same stream simply runs behind it. */
typedef struct {
    const int32_t *auction;           /* device */
    const uint64_t *num;              /* device */
    const int64_t *win_out_offsets;   /* host, n_windows + 1 */
    const uint64_t *win_max;          /* host, n_windows: MAX(num) per window (0 = empty window) */
    const uint64_t *win_groups;       /* host, n_windows: number of distinct auctions per window */
    int64_t rows;
} flockgpu_q5_result;
int flockgpu_q5_hot_items(flockgpu_ctx *ctx, const flockgpu_bid_cols *bid, const flockgpu_windows *win,
                          flockgpu_q5_result *out);

/* q5 as the two stages of q5.dag around the hash repartition (the key-partitioned exchange of a multi-GPU run):
 *   partial  : HashAggregateExec mode=Partial gby=[auction] COUNT(1), PER PANE -- the groups of pane p are rows
 *              [pane_out_offsets[p], pane_out_offsets[p+1]) of (auction, count); windows are not used, only the panes
 *   weighted : the FinalPartitioned side + MAX + join of flockgpu_q5_hot_items over rows that each carry a count (the
 *              partial groups this partition received); the sum of `count` over a window must stay below 2^32.
 * partial on N row-stripes, repartition of the groups by auction, weighted on what arrives == hot_items on all rows. */
typedef struct {
    const int32_t *auction;            /* device, ctx-owned */
    const uint32_t *count;             /* device, ctx-owned */
    const int64_t *pane_out_offsets;   /* host, n_panes + 1 */
    int64_t rows;
} flockgpu_q5_partial_result;
int flockgpu_q5_partial_counts(flockgpu_ctx *ctx, const flockgpu_bid_cols *bid, const flockgpu_windows *win,
                               flockgpu_q5_partial_result *out);
int flockgpu_q5_hot_items_weighted(flockgpu_ctx *ctx, const int32_t *auction, const uint32_t *count, int64_t rows,
                                   const flockgpu_windows *win, flockgpu_q5_result *out);

/* ---- q7 (SURVEY.md section 8(f) "next" query): bid JOIN (SELECT MAX(price) AS maxprice FROM bid) ON price = maxprice,
 * Projection [auction, price, bidder, b_date_time] (benchmarks/src/nexmark/query/q7.sql, q7_plan.fmt), per
 * Tumbling(10 s) window (benchmarks/src/nexmark/main.rs:119).  Every row that reaches the window's maximum is returned
 * (ties kept), in input order; an empty window (MAX = NULL) returns nothing.  win_max: HOST array, the maximum per
 * window (INT32_MIN for an empty window). */
typedef struct {
    const int32_t *auction, *price, *bidder; /* device */
    const int64_t *b_date_time;              /* device */
    const int64_t *win_out_offsets;          /* host, n_windows + 1 */
    const int64_t *win_max;                  /* host, n_windows */
    int64_t rows;
} flockgpu_q7_result;
int flockgpu_q7_highest_bid(flockgpu_ctx *ctx, const flockgpu_bid_cols *bid, const flockgpu_windows *win,
                            flockgpu_q7_result *out);

/* ---- q4 / q9 (SURVEY.md section 8(f) "next" queries), per ElementWise window (benchmarks/src/nexmark/main.rs:117):
 *   Q  = SELECT a_id [, category], MAX(price) AS final FROM auction INNER JOIN bid ON a_id = auction
 *        WHERE b_date_time BETWEEN a_date_time AND expires GROUP BY a_id [, category]
 *   q9 = bid JOIN Q ON auction = id AND price = final -> [auction, bidder, price, b_date_time]  (q9.sql, q9_plan.fmt)
 *   q4 = SELECT category, AVG(final) FROM Q GROUP BY category -> [category Int32, AVG Float64]   (q4.sql)
 * Auction ids must be strictly increasing over a dense range inside every window (the generator's order);
 * otherwise FLOCKGPU_ERR_UNSUPPORTED and the host keeps its own engine for that input.  q9 rows keep input order;
 * q4 rows are ordered by category inside a window. */
typedef struct { /* Auction::schema projection of q4 / q9 (q9_plan.fmt: [0, 5, 6]; q4 adds category) */
    const int32_t *a_id, *category; /* category may be NULL for q9 */
    const int64_t *a_date_time, *expires;
    int64_t rows;
} flockgpu_auction_time_cols;
typedef struct {
    const int32_t *auction, *price, *bidder; /* device */
    const int64_t *b_date_time;              /* device */
    const int64_t *win_out_offsets;          /* host, n_windows + 1 */
    int64_t rows;
} flockgpu_q9_result;
typedef struct {
    const int32_t *category;        /* device */
    const double *avg_final;        /* device */
    const int64_t *win_out_offsets; /* host, n_windows + 1 */
    int64_t rows;
} flockgpu_q4_result;
int flockgpu_q9_winning_bids(flockgpu_ctx *ctx, const flockgpu_auction_time_cols *auction, const flockgpu_windows *auction_win,
                             const flockgpu_bid_cols *bid, const flockgpu_windows *bid_win, flockgpu_q9_result *out);
int flockgpu_q4_avg_final_by_category(flockgpu_ctx *ctx, const flockgpu_auction_time_cols *auction,
                                      const flockgpu_windows *auction_win, const flockgpu_bid_cols *bid,
                                      const flockgpu_windows *bid_win, flockgpu_q4_result *out);

/* ---- q13 (SURVEY.md section 8(f) "next" query): bid JOIN side_input ON auction = key ->
 * [auction, bidder, price, b_date_time, value] (benchmarks/src/nexmark/query/q13.sql, q13_plan.fmt; side_input schema
 * flock/src/datasource/nexmark/event.rs:375-388), per ElementWise window.  The side input (device pointers, any keys,
 * duplicates allowed) is the same for every window.  Rows are ordered by bid row; bid_row / side_row name the joined
 * input rows. */
typedef struct {
    const int32_t *auction, *bidder, *price; /* device */
    const int64_t *b_date_time;              /* device */
    const int32_t *value;                    /* device */
    const int32_t *bid_row, *side_row;       /* device */
    const int64_t *win_out_offsets;          /* host, n_windows + 1 */
    int64_t rows;
} flockgpu_q13_result;
int flockgpu_q13_side_join(flockgpu_ctx *ctx, const flockgpu_bid_cols *bid, const flockgpu_windows *win,
                           const int32_t *side_key, const int32_t *side_value, int64_t side_rows, flockgpu_q13_result *out);

/* ---- q8: DISTINCT (p_id, name) JOIN DISTINCT seller ON p_id = seller -> [p_id, name]
 * (q8.sql, q8_plan.fmt:1-10, q8.dag).  Output grouped by window, ordered by person row. */
typedef struct {
    const int32_t *p_id;              /* device */
    flockgpu_utf8 name;               /* device */
    const int32_t *person_row;        /* device */
    const int64_t *win_out_offsets;   /* host, n_windows + 1 */
    int64_t rows;
    int64_t name_bytes;
} flockgpu_q8_result;
int flockgpu_q8_join(flockgpu_ctx *ctx, const flockgpu_person_cols *person, const flockgpu_windows *person_win,
                     const flockgpu_auction_cols *auction, const flockgpu_windows *auction_win,
                     flockgpu_q8_result *out);

/* ---- asynchronous calls.  The reference runs every plan of a function on its own tokio task and joins them
 * (flock/src/runtime/context.rs:172-191); a synchronous call here leaves the GPU idle while the host prepares the next one and
 * wakes up from its wait (~0.09 ms of q5's 0.94 ms step, a third of q3's 0.10 ms at 1e8 events).  Every ctx owns one worker thread
 * (started on first use).  A `*_async` entry point copies its argument structs, hands the call to the worker and returns;
 * flockgpu_ctx_wait blocks until the call has finished and returns ITS status, with `out` filled exactly as by the synchronous
 * call.  One call in flight per ctx -- a second submit before the wait is FLOCKGPU_ERR_INVALID; the arrays the arguments point to
 * (device columns, window schedules, literals, `out`) are borrowed until the wait returns, and the ctx must not be used in
 * between.  Calls on DIFFERENT ctxs (different streams) are in flight together. */
int flockgpu_q3_join_async(flockgpu_ctx *ctx, const flockgpu_auction_cols *auction, const flockgpu_windows *auction_win,
                           const flockgpu_person_cols *person, const flockgpu_windows *person_win,
                           int64_t category_lit, const char *const *state_lits, int n_state_lits,
                           flockgpu_q3_result *out);
int flockgpu_q5_hot_items_async(flockgpu_ctx *ctx, const flockgpu_bid_cols *bid, const flockgpu_windows *win,
                                flockgpu_q5_result *out);
int flockgpu_q8_join_async(flockgpu_ctx *ctx, const flockgpu_person_cols *person, const flockgpu_windows *person_win,
                           const flockgpu_auction_cols *auction, const flockgpu_windows *auction_win,
                           flockgpu_q8_result *out);
int flockgpu_ctx_wait(flockgpu_ctx *ctx);

/* ---- key-partitioned exchange (the RepartitionExec Hash([key], n) step of the distributed plans,
 * flock/src/distributed_plan/planner.rs:152-171; row routing restated from
 * playground/src/distributed_plan/shuffle_writer.rs:106-148).  The reference hashes with ahash seeds (0,0,0,0);
 * which partition a key lands on is unobservable in query results, so a fixed integer mix is used:
 *   part(key) = (murmur3_fmix32((uint32_t)key) * n_parts) >> 32.
 * Result: the row numbers of every row that lies inside a window, grouped by (partition, window) -- partition
 * major -- with input order kept inside a group, so that `take` over them yields send buffers that are contiguous
 * per destination (one all-to-all chunk) and per window inside a destination.  part_win_offsets is a HOST array of
 * n_parts * n_windows + 1 offsets into `row` (arena-owned, valid until the next call on this ctx). */
typedef struct {
    const int32_t *row;              /* device */
    const int64_t *part_win_offsets; /* host */
    int64_t rows;
} flockgpu_partition_result;
int flockgpu_partition_by_key(flockgpu_ctx *ctx, const int32_t *keys /* device, 16-byte aligned */, int64_t rows,
                              const flockgpu_windows *win, int32_t n_parts, flockgpu_partition_result *out);

/* `take` (arrow::compute::take as used by shuffle_writer.rs:131-141 and by HashJoinExec): out[i] = src[rows[i]].
 * All pointers are device pointers; `out` of the fixed-width variants is caller-allocated (n entries).
 * take_utf8 writes into ctx-arena buffers keyed by `slot` (0..15: one slot per column that must stay alive). */
int flockgpu_take_i32(flockgpu_ctx *ctx, const int32_t *src, const int32_t *rows, int64_t n, int32_t *out);
int flockgpu_take_i64(flockgpu_ctx *ctx, const int64_t *src, const int32_t *rows, int64_t n, int64_t *out);
int flockgpu_take_utf8(flockgpu_ctx *ctx, const flockgpu_utf8 *src, const int32_t *rows, int64_t n, int32_t slot,
                       flockgpu_utf8 *out, int64_t *out_bytes);
/* In-place inclusive prefix sum (rebuilds Arrow Utf8 offsets from received value lengths). */
int flockgpu_inclusive_scan_i32(flockgpu_ctx *ctx, int32_t *data /* device */, int64_t n);

/* ---- q11, user sessions: Window::Session(timeout) keyed by bidder
 * (benchmarks/src/nexmark/main.rs:120,346-349), the launcher's session walk over a run of epochs
 * (flock-function/src/aws/window/session.rs:64-178,205-262) and, per closed session,
 *   SELECT bidder, COUNT(*) AS bid_count, MIN(b_date_time) AS start_time, MAX(b_date_time) AS end_time
 *   FROM bid GROUP BY bidder                                        (benchmarks/src/nexmark/query/q11.sql)
 * Epoch t = rows [epoch_row_offsets[t], epoch_row_offsets[t+1]) of `bid` (only bidder and b_date_time are read;
 * b_date_time must be >= 0).  A bidder's bids of one epoch join its open session unless the first of them lies more
 * than `timeout_s` whole seconds after the session's last bid; after every epoch t the sessions whose last bid is more
 * than `timeout_s` whole seconds older than  base_time_ms/1000 + t  are closed.  Output: the sessions closed in epoch t
 * are rows [epoch_out_offsets[t], epoch_out_offsets[t+1]), ordered by bidder; two sessions of one bidder closed in
 * the same epoch are one row (the query groups by bidder); sessions still open after the last epoch are not reported. */
typedef struct {
    int32_t *bidder;                  /* device, ctx-owned */
    uint64_t *bid_count;              /* COUNT(*) -> UInt64 */
    int64_t *start_time, *end_time;   /* Timestamp(ms) */
    const int64_t *epoch_out_offsets; /* host, n_epochs + 1 */
    int64_t rows;
    int64_t sessions_total;           /* every session found, reported or not */
} flockgpu_q11_result;
int flockgpu_q11_user_sessions(flockgpu_ctx *ctx, const flockgpu_bid_cols *bid, const int64_t *epoch_row_offsets /* host */,
                               int32_t n_epochs, int32_t timeout_s, int64_t base_time_ms, flockgpu_q11_result *out);

/* Rows grouped by key, arrival order kept inside a key -- the `repartition(.., HashDiff([key], distinct))` of the session
 * and global windows (flock-function/src/aws/window/session.rs:242-250): out_keys[i] = keys[out_rows[i]], ascending,
 * stable.  `keys` is a 16-byte aligned device column; the outputs are ctx-owned device arrays of `rows` entries. */
int flockgpu_group_rows_by_key(flockgpu_ctx *ctx, const int32_t *keys, int64_t rows, int32_t **out_keys, int32_t **out_rows);

/* ---- event-time panes: a batch of rows cut into the panes of a hopping window by a timestamp column, on the device -- what WindowSchedule
 * does on the host from the generator's epoch structure, for rows that carry nothing but a timestamp (decoded text).  The rules are
 * A-PN1..11 in csrc/panes.hpp.
 *   pane(t) = floor((t - origin_ms) / hop_ms), rounding towards minus infinity, the difference formed exactly; a pane id outside Int64 is
 *   FLOCKGPU_ERR_INVALID.
 * *first_pane = the smallest pane id present, *n_panes = the largest minus the smallest plus 1 (panes in between that hold no row included);
 * bounds[0] = 0 <= bounds[1] <= ... <= bounds[*n_panes] = rows (host, room for capacity + 1 entries).  rows == 0: *n_panes = 0, *first_pane = 0.
 * Rows in pane order (pane ids never decrease along the rows; timestamps inside a pane in any order -- a time-ordered stream):
 *   *row_list = NULL and pane *first_pane + k is rows [bounds[k], bounds[k + 1]) of the input itself.  One streaming pass over the 8 bytes a row
 *   (and the validity bytes), one small launch for the bounds, two host waits; no division per row.
 * Otherwise *row_list (device, ctx-owned, valid until the next call on the context) is a stable permutation: pane *first_pane + k is the input
 *   rows row_list[bounds[k] .. bounds[k + 1]), ascending inside the pane.
 * `time_ms` needs 8-byte alignment, `valid` (one byte per row, 0 = NULL; NULL pointer: no NULLs) none.
 *   FLOCKGPU_ERR_INVALID      hop_ms <= 0, capacity outside [1, 65536], rows outside [0, 2^31), null pointers, a validity byte of 0 (the message
 *                             names the first such row, 0-based), a pane id outside Int64;
 *   FLOCKGPU_ERR_UNSUPPORTED  more than `capacity` panes (the message names the first pane id, the last pane id and the capacity).
 * A refused call writes nothing to `bounds`. */
int flockgpu_pane_split(flockgpu_ctx *ctx, const int64_t *time_ms /* device */, const uint8_t *valid /* device, or NULL */,
                        int64_t rows, int64_t origin_ms, int64_t hop_ms, int32_t capacity,
                        int64_t *first_pane, int32_t *n_panes, int64_t *bounds /* host, capacity + 1 */,
                        const int32_t **row_list /* device, ctx-owned; NULL when the rows are in pane order */);
/* out[i] = src[rows[i]] for one-byte values (validity bytes at a row list); `rows` is 16-byte aligned, `out` caller-allocated. */
int flockgpu_take_u8(flockgpu_ctx *ctx, const uint8_t *src, const int32_t *rows, int64_t n, uint8_t *out);

/* ---- JSON lines -> columns (the decode step of `select_event_to_batches`,
 * flock/src/datasource/nexmark/nexmark.rs:180-205): the reference keeps an epoch's events as newline-delimited
 * serde_json objects (generator.rs:79-93) and decodes them with arrow's json::Reader against the relation's schema
 * (`event_bytes_to_batch`, flock/src/transmute.rs:255-266).  Every line is one object; members are matched to `fields`
 * by name in any order, other members are checked against the whole JSON grammar and dropped; row = line.  Int32 / Int64
 * fields take JSON integer literals (a Timestamp(ms) column is Int64 here), Utf8 fields take strings (all escapes, \uXXXX
 * surrogate pairs included; bytes >= 0x80 are copied as they are, nothing checks that they are UTF-8).  The rules are
 * A-JSON1..9 at the top of csrc/json.hip.  Errors name the first offending line ("json: line N: ..."):
 *   FLOCKGPU_ERR_INVALID      malformed JSON anywhere in the line (in a dropped member as well, "1x" or "1." for an integer
 *                             included), a missing field, a value of the wrong type, an integer outside its type;
 *   FLOCKGPU_ERR_UNSUPPORTED  well-formed JSON that the decoder declines: a blank line, an escape inside a KEY of the line's
 *                             object, an integer field written with a well-formed fraction / exponent ("1.5", "1e3"), brackets
 *                             nested more than 64 deep inside a dropped member; also more than 16 fields or a name that is
 *                             empty or longer than 31 bytes.
 * `json`: device text, 16-byte aligned, below 2^31 bytes per call. */
enum { FLOCKGPU_JSON_INT32 = 0, FLOCKGPU_JSON_INT64 = 1, FLOCKGPU_JSON_UTF8 = 2 };
typedef struct {
    const char *name; /* host, at most 31 bytes */
    int32_t type;     /* FLOCKGPU_JSON_* */
} flockgpu_json_field;
typedef struct {
    void *values;       /* device, ctx-owned: int32_t / int64_t per row (NULL for a Utf8 field) */
    flockgpu_utf8 utf8; /* device, ctx-owned: offsets (rows + 1) and bytes of a Utf8 field */
    int64_t utf8_bytes;
} flockgpu_json_column;
int flockgpu_json_lines_decode(flockgpu_ctx *ctx, const uint8_t *json /* device */, int64_t n_bytes, const flockgpu_json_field *fields,
                               int32_t n_fields, flockgpu_json_column *out /* n_fields */, int64_t *rows);

/* ---- Delimited text -> columns (csv.hip): the reference's other text format -- q13's side input (arrow's csv::ReaderBuilder with
 * has_header(true), with_delimiter(b','), flock-function/src/aws/actor.rs:575-629) and the TPC-H '.tbl' files (CsvReadOptions with
 * delimiter(b'|'), playground/src/distributed_plan/partition.rs:157-179).  `fields` has one entry per column OF THE FILE, in file order;
 * SKIP columns are walked and not parsed (a '.tbl' line ends in '|': declare one more SKIP column for it).  Records end at \n or \r\n
 * outside quotes; a field that begins with '"' is quoted, '""' inside is one '"'.  An empty field is NULL for a numeric column
 * (valid[i] = 0, value 0) and '' for Utf8.  Float64 is converted only where one IEEE operation is exact-then-correctly-rounded (at most
 * 2^53 as significand, a decimal exponent in [-22, 22]) and refused outside.  The full rules: A-CSV1..7 in flock_amd/csrc/csv.hpp.
 * Errors name the first offending record (1-based, the header counted), the column and its type: malformed quoting, a wrong field count,
 * a value that does not parse -> FLOCKGPU_ERR_INVALID; a blank line, a bare \r, a Float64 outside the exact range ->
 * FLOCKGPU_ERR_UNSUPPORTED.  Outputs are ctx-owned and valid until the next call on the context.  `text`: device, 16-byte aligned, below
 * 2^31 bytes; no byte at or past text + n_bytes is read.  n_fields <= 64. */
enum { FLOCKGPU_CSV_SKIP = -1, FLOCKGPU_CSV_INT32 = 0, FLOCKGPU_CSV_INT64 = 1, FLOCKGPU_CSV_UINT64 = 2,
       FLOCKGPU_CSV_FLOAT64 = 3, FLOCKGPU_CSV_TIMESTAMP_MS = 4, FLOCKGPU_CSV_UTF8 = 5 };
typedef struct {
    int32_t type; /* FLOCKGPU_CSV_* */
} flockgpu_csv_field;
typedef struct {
    uint8_t delimiter;  /* any ASCII byte except '"', \r and \n */
    int32_t has_header; /* non-zero: the first record is dropped unread */
} flockgpu_csv_options;
typedef struct {
    void *values;       /* device: int32_t / int64_t / uint64_t / double per row (NULL for Utf8) */
    uint8_t *valid;     /* device: one byte per row, 1 = not NULL; always written for numeric columns (NULL for Utf8) */
    int64_t null_count; /* rows whose valid byte is 0 */
    flockgpu_utf8 utf8; /* device: offsets (rows + 1) and bytes of a Utf8 column */
    int64_t utf8_bytes;
} flockgpu_csv_column;
int flockgpu_csv_decode(flockgpu_ctx *ctx, const uint8_t *text /* device, 16-byte aligned */, int64_t n_bytes,
                        const flockgpu_csv_field *fields, int32_t n_fields, const flockgpu_csv_options *opt,
                        flockgpu_csv_column *out /* n_fields; untouched for SKIP */, int64_t *rows);

/* ---- Columns -> text (textenc.hip): the way back from the two decoders.  flockgpu_json_lines_encode writes what the reference's generator
 * keeps per epoch -- serde_json::to_vec(event) + "\n" (flock/src/datasource/nexmark/generator.rs:79-93): {"name":value,...}\n per row, the
 * columns in the given order, no white space; strings with serde_json's escapes (\" \\ \b \f \n \r \t, \u00xx for the other bytes below 0x20,
 * everything else verbatim), NULL as null, a Timestamp(ms) as its integer.  flockgpu_csv_encode writes what flockgpu_csv_decode reads:
 * fields joined by the delimiter, records ended by \n, a header record of the names when opt->has_header; a Utf8 value is quoted when it is
 * empty or holds the delimiter, '"', \n or \r ('"' doubled); a Timestamp(ms) prints as YYYY-MM-DD HH:MM:SS[.mmm]; NULL of any type is an empty
 * unquoted field (so a NULL Utf8 reads back as ''), and a record that would be empty is written "".  Integers print in their shortest decimal
 * form.  The full rules: A-ENC1..10 in flock_amd/csrc/textenc.hpp.
 *   FLOCKGPU_ERR_UNSUPPORTED  a Float64 column, more than 64 columns, a name that is empty or longer than 31 bytes (each names the column);
 *                             a text of 2^31 - 16 bytes or more;
 *   FLOCKGPU_ERR_INVALID      no columns, a bad delimiter, rows < 0 or >= 2^31, a Utf8 column without offsets; CSV only: a non-NULL
 *                             Timestamp(ms) outside the years 0000..9999 -- the message names the first such record (1-based, the header
 *                             counted) and the column.
 * Columns may alias each other.  No byte at or past the end of a column is read.  out->text is ctx-owned, 16-byte aligned, valid until the
 * next call on the context; its allocation is a multiple of 16 bytes with zeros behind n_bytes: both decoders read it in place. */
enum { FLOCKGPU_TEXT_INT32 = 0, FLOCKGPU_TEXT_INT64 = 1, FLOCKGPU_TEXT_UINT64 = 2,
       FLOCKGPU_TEXT_FLOAT64 = 3, FLOCKGPU_TEXT_TIMESTAMP_MS = 4, FLOCKGPU_TEXT_UTF8 = 5 };   /* the CSV decoder's numbering */
typedef struct {
    const char *name;     /* host; JSON key / CSV header cell, 1 .. 31 bytes */
    int32_t type;         /* FLOCKGPU_TEXT_* */
    const void *values;   /* device: int32_t / int64_t / uint64_t per row (NULL for Utf8) */
    const uint8_t *valid; /* device, one byte per row, 1 = not NULL; NULL pointer = no NULLs */
    flockgpu_utf8 utf8;   /* device: offsets (rows + 1) and bytes of a Utf8 column */
} flockgpu_text_column;
typedef struct {
    uint8_t *text;   /* device, ctx-owned */
    int64_t n_bytes;
} flockgpu_text_result;
int flockgpu_json_lines_encode(flockgpu_ctx *ctx, const flockgpu_text_column *cols, int32_t n_cols, int64_t rows, flockgpu_text_result *out);
int flockgpu_csv_encode(flockgpu_ctx *ctx, const flockgpu_text_column *cols, int32_t n_cols, int64_t rows,
                        const flockgpu_csv_options *opt /* delimiter; has_header: write one */, flockgpu_text_result *out);

/* ---- JSON lines -> columns with NULLs (json.hip): reads what flockgpu_json_lines_encode writes, and what writers other than serde_json
 * produce -- `null` and members that are simply not there.  An entry point BESIDE flockgpu_json_lines_decode, whose rules, messages and
 * kernels stay as they are.  Lines, grammar, dropped members, repeated keys (the last occurrence wins), verbatim bytes, error order and the
 * limits (1 .. 16 fields, names of 1 .. 31 bytes, "json: line N: ...") are flockgpu_json_lines_decode's.  What is new (A-JSONN1..7 at the
 * top of csrc/json.hip):
 *   - every field is required (nullable = 0: exactly the first entry point's behaviour, null or absence is FLOCKGPU_ERR_INVALID with its
 *     messages) or nullable: the literal null, and a line that lacks the member, give a NULL -- valid[i] = 0 and value 0; a Utf8 NULL is a
 *     value of length 0 with valid[i] = 0, "" one with valid[i] = 1.  {} is a row of NULLs when every field is nullable;
 *   - the encoders' six types, FLOCKGPU_TEXT_*: Timestamp(ms) is a JSON integer in Int64's range, UInt64 an integer literal in
 *     0 .. 18446744073709551615 (a '-' in front, "-0" included, is out of range), Float64 a JSON number that is converted only inside
 *     flockgpu_csv_decode's exact range (a significand of at most 2^53, a decimal exponent in [-22, 22]; "3" is 3.0, "-0.0" is -0.0) and
 *     refused outside it with FLOCKGPU_ERR_UNSUPPORTED, the message naming the line and the field;
 *   - true, false, a string for a number, a number for a string, nul, NULL, nullx: FLOCKGPU_ERR_INVALID; an integer field with a well-formed
 *     fraction / exponent and a blank line stay FLOCKGPU_ERR_UNSUPPORTED.
 * `valid` (one byte per row, 1 = not NULL) is written for every nullable field, Utf8 included, and is a null pointer for a required one;
 * null_count is filled per column.  Outputs are ctx-owned and valid until the next call on the context.  `json`: device text, 16-byte
 * aligned, below 2^31 - 16 bytes; no byte at or past json + n_bytes is read. */
typedef struct {
    const char *name; /* host, 1 .. 31 bytes */
    int32_t type;     /* FLOCKGPU_TEXT_* */
    int32_t nullable; /* non-zero: null and an absent member are NULL */
} flockgpu_json_nfield;
typedef struct {
    void *values;       /* device: int32_t / int64_t / uint64_t / double per row (NULL for Utf8) */
    uint8_t *valid;     /* device: one byte per row, 1 = not NULL (NULL pointer for a required field) */
    int64_t null_count; /* rows whose valid byte is 0 */
    flockgpu_utf8 utf8; /* device: offsets (rows + 1) and bytes of a Utf8 field */
    int64_t utf8_bytes;
} flockgpu_json_ncolumn;
int flockgpu_json_lines_decode_nullable(flockgpu_ctx *ctx, const uint8_t *json /* device, 16-byte aligned */, int64_t n_bytes,
                                        const flockgpu_json_nfield *fields, int32_t n_fields, flockgpu_json_ncolumn *out /* n_fields */,
                                        int64_t *rows);

/* ---- Arrow IPC body assembly: the body of the Arrow Flight data the reference builds for
 * every output batch (`flight_data_from_arrow_batch`, flock/src/transmute.rs:155-170,190-205; `Payload`,
 * flock/src/runtime/payload.rs:118-192) = the batch's buffers in field order, each padded with zeros to 8 bytes.
 * `buffers[i]` are device buffers (bytes = 0: an absent validity bitmap, contributes nothing); `out` is a device buffer
 * of `out_capacity` bytes (NULL: only the size is returned).  The header next to it is written on the host
 * (flock_amd/payload.py); compression stays on the CPU as in the reference (flock/src/encoding.rs:57-100). */
typedef struct {
    const void *data; /* device */
    int64_t bytes;
} flockgpu_ipc_buffer;
int flockgpu_ipc_pack_body(flockgpu_ctx *ctx, const flockgpu_ipc_buffer *buffers, int32_t n_buffers, uint8_t *out /* device */,
                           int64_t out_capacity, int64_t *out_bytes);

/* ---- Yahoo Streaming Benchmark: per Tumbling(10 s) window (benchmarks/src/ysb/main.rs:91)
 *   SELECT campaign_id, COUNT(*) FROM ad_event INNER JOIN campaign ON ad_id = c_ad_id WHERE event_type = lit
 *   GROUP BY campaign_id         (benchmarks/src/ysb/ysb.sql; flock/src/distributed_plan/planner.rs:298-346)
 * Columns are the projections of AdEvent / Campaign the query scans (flock/src/datasource/ysb/event.rs:24-87), Arrow Utf8.
 * Keys and the literal may be up to 40 bytes (UUIDs are 36); longer values -> FLOCKGPU_ERR_UNSUPPORTED.  Output rows:
 * (campaign_id Utf8, COUNT UInt64) of every campaign with at least one matching event, grouped by window. */
typedef struct {
    flockgpu_utf8 ad_id, event_type;
    int64_t rows;
} flockgpu_ysb_event_cols;
typedef struct {
    flockgpu_utf8 c_ad_id, campaign_id;
    int64_t rows;
} flockgpu_ysb_campaign_cols;
typedef struct {
    flockgpu_utf8 campaign_id;      /* device */
    const uint64_t *count;          /* device */
    const int64_t *win_out_offsets; /* host, n_windows + 1 */
    int64_t rows;
    int64_t campaign_bytes;
} flockgpu_ysb_result;
int flockgpu_ysb_campaign_counts(flockgpu_ctx *ctx, const flockgpu_ysb_event_cols *events, const flockgpu_windows *win,
                                 const flockgpu_ysb_campaign_cols *campaigns, const char *event_type_lit,
                                 flockgpu_ysb_result *out);
/* Device-side YSB source (flock/src/datasource/ysb/generator.rs:38-101 restated; every value is a pure function of
 * (seed, index): ysb_gen.hip).  Offsets arrays have rows + 1 entries; ad-id / campaign-id byte buffers hold 36 bytes per
 * row, the event_type buffer up to 8 bytes per event. */
int flockgpu_ysb_gen_campaigns(flockgpu_ctx *ctx, uint64_t seed, int64_t n_campaigns, int64_t ads, int32_t *c_ad_id_off,
                               uint8_t *c_ad_id_bytes, int32_t *campaign_off, uint8_t *campaign_bytes);
int flockgpu_ysb_gen_events(flockgpu_ctx *ctx, uint64_t seed, uint64_t first_event, int64_t n_events, int64_t n_ads,
                            int32_t *ad_id_off, uint8_t *ad_id_bytes, int32_t *event_type_off, uint8_t *event_type_bytes);

/* ---- device-side NEXMark source (flock/src/datasource/nexmark/{event,config,generator}.rs restated,
 * deviations D1-D4 documented in DESIGN.md).  Generates the columns the five plans scan for event
 * numbers [n0, n1) of a stream straight into HBM; any output pointer may be NULL to skip it. */
typedef struct {
    uint64_t seed, first_event_id, eps, base_time;
} flockgpu_nexmark_stream;
int flockgpu_nexmark_counts(const flockgpu_nexmark_stream *s, uint64_t n0, uint64_t n1,
                            uint64_t *n_person, uint64_t *n_auction, uint64_t *n_bid);
int flockgpu_nexmark_gen_bids(flockgpu_ctx *ctx, const flockgpu_nexmark_stream *s, uint64_t n0, uint64_t n1,
                              int32_t *auction, int32_t *bidder, int32_t *price, int64_t *b_date_time);
int flockgpu_nexmark_gen_auctions(flockgpu_ctx *ctx, const flockgpu_nexmark_stream *s, uint64_t n0, uint64_t n1,
                                  int32_t *a_id, int32_t *seller, int32_t *category);
int flockgpu_nexmark_gen_auction_times(flockgpu_ctx *ctx, const flockgpu_nexmark_stream *s, uint64_t n0, uint64_t n1,
                                       int64_t *a_date_time, int64_t *expires);
/* Persons: offsets arrays have rows + 1 entries; byte buffers must hold rows*14 / rows*13 / rows*2. */
int flockgpu_nexmark_gen_persons(flockgpu_ctx *ctx, const flockgpu_nexmark_stream *s, uint64_t n0, uint64_t n1,
                                 int32_t *p_id, int32_t *name_off, uint8_t *name_bytes, int32_t *city_off,
                                 uint8_t *city_bytes, int32_t *state_off, uint8_t *state_bytes);

#ifdef __cplusplus
}
#endif
#endif /* FLOCKGPU_H */
