// Plan-level C ABI (include/flockgpu_plan.h), the ingest half: Arrow C Data Interface batches into a plan's leaves.
//   feed_data_sources  flock/src/runtime/context.rs:257-325   -> flockgpu_plan_feed (pinned or staged H2D, no host wait)
//   clean_data_sources context.rs:227-254                     -> flockgpu_plan_reset
// and what this library adds to it: the device-side pane ring (flockgpu_plan_ring_*, flockgpu_plan_feed_pane), the prefetch of the next
// pane (flockgpu_plan_prefetch_pane), leaves that read another plan's relation or result in place (flockgpu_plan_feed_shared / _from).
// At the end: device columns into a leaf, as a whole feed or as a pane of the ring, and a retained result out as device columns
// (flockgpu_plan_feed_columns / _feed_pane_columns / _result_columns; the kernels are plan_source.hip's).
// Host-side code only.  Each decision has one owner: check_feed / apply_feed (what a feed is, and doing it), match_schema / check_column
// (a fed batch against the leaf), reserve_rows (room for an append), add_run / issue_runs (what travels as one copy, and how).
#include <memory>
#include <thread>

#include "plan_source.hpp"
#include "plan_state.hpp"

using namespace flockgpu;
using namespace flockgpu::ir;
using namespace flockgpu::plan_detail;

namespace {

// ------------------------------------------------------------------ feeding
int find_child(const ArrowSchema *schema, const std::string &name) {
    for (int64_t i = 0; i < schema->n_children; ++i)
        if (schema->children[i] && schema->children[i]->name && name == schema->children[i]->name) return (int)i;
    return -1;
}
bool format_ok(const Field &f, const char *got) {
    if (!got) return false;
    if (f.is_ts) return !strncmp(got, "tsm:", 4) || !strcmp(got, "l");
    switch (f.type) {
        case ColType::I32: return !strcmp(got, "i");
        case ColType::I64: return !strcmp(got, "l") || !strncmp(got, "tsm:", 4);
        case ColType::U64: return !strcmp(got, "L");
        case ColType::F64: return !strcmp(got, "g");
        default: return !strcmp(got, "u");
    }
}

// Device buffer that keeps its contents when it grows (append-only feeding).
int grow(flockgpu_ctx *ctx, const std::string &key, size_t keep_bytes, size_t want_bytes, void **ptr) {
    DeviceBuf &b = ctx->arena[key];
    if (b.cap >= want_bytes && b.ptr) { *ptr = b.ptr; return FLOCKGPU_OK; }
    size_t cap = std::max<size_t>(want_bytes + want_bytes / 2, 1024);
    cap = (cap + 255) & ~size_t(255);
    if (guard_arena()) cap = want_bytes;   // (experimental builds: exactly what was asked for, at the end of mapped memory)
    void *np = nullptr;
    hipError_t e = dev_alloc(ctx, &np, cap);
    if (e != hipSuccess) return fail(ctx, FLOCKGPU_ERR_OOM, "plan feed: hipMalloc(%zu): %s", cap, hipGetErrorString(e));
    if (b.ptr) {
        if (keep_bytes) {
            e = hipMemcpyAsync(np, b.ptr, keep_bytes, hipMemcpyDeviceToDevice, ctx->stream);
            if (e != hipSuccess) { dev_free(ctx, np); return fail(ctx, FLOCKGPU_ERR_HIP, "plan feed: grow copy: %s", hipGetErrorString(e)); }
        }
        (void)hipStreamSynchronize(ctx->stream);
        dev_free(ctx, b.ptr);
    }
    b.ptr = np;
    b.cap = cap;
    *ptr = np;
    return FLOCKGPU_OK;
}

bool host_is_pinned(const void *p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // pageable memory: the query fails and leaves a sticky error behind
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// A transfer that continues an open run (source and destination both contiguous: the batches of a relation are often slices of one allocation --
// the reference's own `event_bytes_to_batch` output is -- and 52 copies of 0.7 MB cost 15 us of set-up each; 26 of them are 0.4 ms on the calling
// thread) is merged into it; anything else starts a run.  Every run is looked at: a feed's columns interleave batch by batch.
void add_run(std::vector<flockgpu_plan::CopyJob> &runs, void *dst, const void *src, size_t bytes) {
    for (auto &r : runs)
        if (static_cast<uint8_t *>(r.dst) + r.bytes == dst && static_cast<const uint8_t *>(r.src) + r.bytes == src) {
            r.bytes += bytes;
            return;
        }
    runs.push_back(flockgpu_plan::CopyJob{dst, src, bytes});
}
// Host -> device on the plan's stream without a host wait: the transfer joins the feed's runs, which go out in flush_jobs().
int h2d(flockgpu_plan *pl, void *dst, const void *src, size_t bytes) {
    if (!bytes) return FLOCKGPU_OK;
    pl->fed_bytes += (int64_t)bytes;
    add_run(pl->runs, dst, src, bytes);
    return FLOCKGPU_OK;
}
// Sends `runs`: pinned (registered) memory straight to the DMA engine on `stream`, pageable memory cut into kStageChunk pieces for the caller's
// staging lanes (`staged`: their bytes).
int issue_runs(flockgpu_ctx *ctx, hipStream_t stream, const std::vector<flockgpu_plan::CopyJob> &runs, std::vector<flockgpu_plan::CopyJob> *pieces,
               size_t *staged) {
    for (auto &r : runs) {
        const uint8_t *src = static_cast<const uint8_t *>(r.src);
        uint8_t *dst = static_cast<uint8_t *>(r.dst);
        // (both ends: a merged run may have grown out of a registered range into pageable memory)
        if (host_is_pinned(src) && host_is_pinned(src + r.bytes - 1)) {
            FG_HIP(ctx, hipMemcpyAsync(dst, src, r.bytes, hipMemcpyHostToDevice, stream));
            continue;
        }
        for (size_t done = 0; done < r.bytes; done += kStageChunk) {
            const size_t n = std::min(kStageChunk, r.bytes - done);
            pieces->push_back(flockgpu_plan::CopyJob{dst + done, src + done, n});
            *staged += n;
        }
    }
    return FLOCKGPU_OK;
}

// One staging lane: its share of the pieces, each copied into one of the lane's two pinned chunks (the host fills one while the
// other is in flight) and sent with hipMemcpyAsync on the plan's stream.  (hipMemcpyAsync from pageable memory would block the
// caller for the whole transfer and moves ~10 GB/s; one host thread's memcpy is no faster -- several lanes side by side are.)
int stage_lane(flockgpu_plan *pl, int lane, const std::vector<flockgpu_plan::CopyJob> &pieces, int n_lanes) {
    flockgpu_ctx *ctx = pl->ctx;
    if (hipSetDevice(ctx->device) != hipSuccess) return FLOCKGPU_ERR_HIP;
    for (size_t i = (size_t)lane; i < pieces.size(); i += (size_t)n_lanes) {
        const int k = lane * 2 + pl->stage_next[lane];
        pl->stage_next[lane] ^= 1;
        if (!pl->stage[k]) {   // a lane's two chunks exist from the lane's first use on (all 16 up front pinned 64 MiB per plan)
            if (hipHostMalloc(&pl->stage[k], kStageChunk, hipHostMallocDefault) != hipSuccess) return FLOCKGPU_ERR_OOM;
            if (hipEventCreateWithFlags(&pl->stage_done[k], hipEventDisableTiming) != hipSuccess) return FLOCKGPU_ERR_HIP;
        } else if (hipEventSynchronize(pl->stage_done[k]) != hipSuccess) {
            return FLOCKGPU_ERR_HIP;
        }
        std::memcpy(pl->stage[k], pieces[i].src, pieces[i].bytes);
        if (hipMemcpyAsync(pieces[i].dst, pl->stage[k], pieces[i].bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return FLOCKGPU_ERR_HIP;
        if (hipEventRecord(pl->stage_done[k], ctx->stream) != hipSuccess) return FLOCKGPU_ERR_HIP;
    }
    return FLOCKGPU_OK;
}

int flush_jobs(flockgpu_plan *pl) {
    flockgpu_ctx *ctx = pl->ctx;
    std::vector<flockgpu_plan::CopyJob> pieces;
    size_t total = 0;
    const int rc_runs = issue_runs(ctx, ctx->stream, pl->runs, &pieces, &total);
    pl->runs.clear();
    FG_TRY(rc_runs);
    if (pieces.empty()) return FLOCKGPU_OK;
    // small feeds stay on the calling thread; from a few MB on the lanes pay for their start-up
    // (2 / 4 / 6 / 8 lanes: 1.12 / 1.09-1.13 / 1.09 / 1.12 ms per 36.8 MB window, round 4 -- the transfer, not the host copy, is what is left)
    constexpr int want_lanes = 4;
    const int n_lanes = total < (size_t(2) << 20) ? 1 : (int)std::min<size_t>((size_t)want_lanes, std::max<size_t>(1, std::thread::hardware_concurrency()));
    std::vector<std::thread> workers;   // (lane 0 is the calling thread)
    std::vector<int> rc((size_t)n_lanes, FLOCKGPU_OK);
    for (int l = 1; l < n_lanes; ++l) workers.emplace_back([&, l] { rc[(size_t)l] = stage_lane(pl, l, pieces, n_lanes); });
    rc[0] = stage_lane(pl, 0, pieces, n_lanes);
    for (auto &w : workers) w.join();
    for (int r : rc)
        if (r != FLOCKGPU_OK) return fail(ctx, FLOCKGPU_ERR_HIP, "plan feed: staged host-to-device copy failed");
    return FLOCKGPU_OK;
}

bool validity_has_nulls(const ArrowArray *a, int64_t offset, int64_t n) {
    if (a->null_count == 0 || a->n_buffers < 1 || !a->buffers[0]) return false;
    if (a->null_count > 0) return true;
    const uint8_t *bits = static_cast<const uint8_t *>(a->buffers[0]);  // null_count == -1: not computed, look at the bitmap
    for (int64_t i = offset; i < offset + n; ++i)
        if (!((bits[i >> 3] >> (i & 7)) & 1)) return true;
    return false;
}

// The columns the leaf reads, as children of the fed schema (-1: not read), matched by name; `who` begins the messages.
int match_schema(flockgpu_ctx *ctx, const char *who, const Leaf &lf, const ArrowSchema *schema, std::vector<int> *child) {
    child->assign(lf.schema.size(), -1);
    for (size_t c = 0; c < lf.schema.size(); ++c) {
        if (!lf.needed[c]) continue;
        const int at = (*child)[c] = find_child(schema, lf.schema[c].name);
        if (at < 0) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: column '%s' missing from the fed schema", who, lf.schema[c].name.c_str());
        if (!format_ok(lf.schema[c], schema->children[at]->format))
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: column '%s' has Arrow format '%s', the plan scans %s", who, lf.schema[c].name.c_str(),
                        schema->children[at]->format, type_name(lf.schema[c]));
    }
    return FLOCKGPU_OK;
}
// Column `f` of batch `rb` (a batch that matches the schema): there, as long as the batch, with the buffers of its type and -- where it has rows -- data.
int check_column(flockgpu_ctx *ctx, const char *who, const Field &f, const ArrowArray *rb, int child) {
    const ArrowArray *a = rb->children[child];
    if (!a || a->length < rb->offset + rb->length) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: column '%s' is shorter than its batch", who, f.name.c_str());
    const bool utf8 = f.type == ColType::UTF8;
    if (a->n_buffers < (utf8 ? 3 : 2) || (rb->length > 0 && !a->buffers[1]))
        return fail(ctx, FLOCKGPU_ERR_INVALID, utf8 ? "%s: Utf8 column '%s' without 3 buffers" : "%s: column '%s' without a data buffer", who, f.name.c_str());
    return FLOCKGPU_OK;
}

}  // namespace

// (the flockgpu_plan_* functions below have C linkage from their declarations in flockgpu_plan.h)
int flockgpu_plan_input_matches(const flockgpu_plan *plan, int input, const struct ArrowSchema *schema) {
    if (!plan || !schema || input < 0 || input >= (int)plan->ir.leaves.size()) return 0;
    const Leaf &lf = plan->ir.leaves[(size_t)input];
    for (size_t c = 0; c < lf.schema.size(); ++c)
        if (lf.needed[c] && find_child(schema, lf.schema[c].name) < 0) return 0;
    return 1;
}

// What check_feed found out about a feed and apply_feed acts on.  Nothing here is a copy of the leaf's cursors: apply_feed reads those when it runs.
struct FeedCheck {
    std::vector<int> child;                   // leaf column -> child of the fed schema (-1: not read)
    std::vector<std::vector<int64_t>> keep;   // per batch: the rows that survive NULL dropping (empty: all)
    std::vector<char> filtered;               // per batch: `keep` applies
    std::vector<char> with_valid;             // (batch, column): NULLs that stay -> validity bytes go along
    int64_t add_rows = 0;
    std::vector<int64_t> add_bytes;           // per Utf8 column
    int scheme_state = -1;                    // the hash-placement guard's state once this feed is in
    std::string scheme_tag;
};

// A leaf's cursors, for a feed that has to go back to them: the buffers keep what was appended behind, nothing counts it any more.
struct LeafSnapshot {
    int64_t rows;
    std::vector<int64_t> bytes;   // per column
    explicit LeafSnapshot(const LeafData &ld) : rows(ld.rows) { for (auto &c : ld.cols) bytes.push_back(c.bytes); }
    void restore(LeafData &ld) const {
        ld.rows = rows;
        for (size_t c = 0; c < ld.cols.size(); ++c) {
            ld.cols[c].bytes = bytes[c];
            ld.cols[c].valid_rows = std::min(ld.cols[c].valid_rows, rows);   // (validity bytes never cover more than the leaf's rows)
        }
    }
};

// feed_data_sources for one leaf, first half: every check of the feed, nothing moved (flockgpu_plan_feed_pane asks before it opens a new
// pane, so that a refused feed leaves the ring as it was).
static int check_feed(flockgpu_plan *plan, int input, const struct ArrowSchema *schema, const struct ArrowArray *const *batches, int n_batches,
                      FeedCheck &chk) {
    flockgpu_ctx *ctx = plan->ctx;
    if (!schema || input < 0 || input >= (int)plan->ir.leaves.size() || n_batches < 0 || (n_batches && !batches))
        return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed: bad argument");
    if (plan->async_pending) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed: an asynchronous execute is in flight (flockgpu_plan_wait first)");
    FG_HIP(ctx, hipSetDevice(ctx->device));
    const Leaf &lf = plan->ir.leaves[(size_t)input];
    LeafData &ld = plan->leaves[(size_t)input];
    if (ld.borrowed) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed: input %d shares another plan's relation; reset the plan first", input);
    // hash placement (flockgpu_plan.h): the co-partitioned inputs of one invocation must all have been placed by the same scheme
    chk.scheme_state = plan->scheme_state;
    chk.scheme_tag = plan->scheme_tag;
    if (lf.co_partitioned) {
        bool any_rows = false;
        for (int b = 0; b < n_batches; ++b) any_rows = any_rows || (batches[b] && batches[b]->length > 0);
        if (any_rows) {
            std::string tag;
            const int tagged = find_metadata(schema->metadata, kPartitionSchemeKey, &tag) ? 1 : 0;
            if (tagged && tag != kPartitionScheme)
                return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed: partitions placed by scheme '%s', this library places by '%s': one key would meet two consumers",
                            tag.c_str(), kPartitionScheme);
            if (chk.scheme_state >= 0 && chk.scheme_state != tagged)
                return fail(ctx, FLOCKGPU_ERR_INVALID,
                            "plan_feed: mixed hash placement -- this stage was fed partitions tagged '%s' and untagged ones (another engine's hash): "
                            "every producer of a stage must place rows the same way", kPartitionScheme);
            chk.scheme_state = tagged;
            chk.scheme_tag = tag;
        }
    }
    FG_TRY(match_schema(ctx, "plan_feed", lf, schema, &chk.child));
    const std::vector<int> &child = chk.child;
    // validate everything before the first copy, so that a rejected feed leaves the leaf as it was
    chk.add_rows = 0;
    chk.add_bytes.assign(lf.schema.size(), 0);
    chk.keep.assign((size_t)n_batches, {});
    chk.filtered.assign((size_t)n_batches, 0);
    chk.with_valid.assign((size_t)n_batches * lf.schema.size(), 0);
    for (int b = 0; b < n_batches; ++b) {
        const ArrowArray *rb = batches[b];
        if (!rb || rb->n_children < schema->n_children) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed: batch %d does not match the schema", b);
        const int64_t n = rb->length;
        if (n == 0) continue;
        for (size_t c = 0; c < lf.schema.size(); ++c) {
            if (child[c] < 0) continue;
            FG_TRY(check_column(ctx, "plan_feed", lf.schema[c], rb, child[c]));
            const ArrowArray *a = rb->children[child[c]];
            const int64_t off = a->offset + rb->offset;
            if (!validity_has_nulls(a, off, n)) continue;
            // NULLs.  Where dropping the row cannot change the result (inner-join keys, columns only compared under AND, MAX arguments of a
            // global aggregate) the row is left out here; everywhere else the column travels with a validity byte per row and the
            // operators honour it (NULLs skipped by COUNT(col) / MIN / MAX / SUM / AVG, one group for NULL keys, NULLs in the output)
            if (!lf.null_droppable[c]) {
                if (plan->ring_ppw && plan->ring_q5)   // (q5's ring keeps Partial COUNT groups of plain columns; the rows ring carries validity along)
                    return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan_feed: column '%s' holds NULLs that reach the output; q5's pane ring keeps no validity", lf.schema[c].name.c_str());
                chk.with_valid[(size_t)b * lf.schema.size() + c] = 1;
                continue;
            }
            const uint8_t *bits = static_cast<const uint8_t *>(a->buffers[0]);
            std::vector<int64_t> &k = chk.keep[(size_t)b];
            if (!chk.filtered[(size_t)b]) {
                k.resize((size_t)n);
                for (int64_t i = 0; i < n; ++i) k[(size_t)i] = i;
                chk.filtered[(size_t)b] = 1;
            }
            size_t w = 0;
            for (int64_t i : k)
                if ((bits[(off + i) >> 3] >> ((off + i) & 7)) & 1) k[w++] = i;
            k.resize(w);
        }
        const int64_t n_keep = chk.filtered[(size_t)b] ? (int64_t)chk.keep[(size_t)b].size() : n;
        for (size_t c = 0; c < lf.schema.size(); ++c) {
            if (child[c] < 0 || lf.schema[c].type != ColType::UTF8) continue;
            const ArrowArray *a = rb->children[child[c]];
            const int32_t *so = static_cast<const int32_t *>(a->buffers[1]) + a->offset + rb->offset;
            if (!chk.filtered[(size_t)b]) chk.add_bytes[c] += (int64_t)so[n] - so[0];
            else for (int64_t i : chk.keep[(size_t)b]) chk.add_bytes[c] += so[i + 1] - so[i];
        }
        chk.add_rows += n_keep;
    }
    if (ld.rows + chk.add_rows >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan_feed: more than 2^31 rows per relation");
    for (size_t c = 0; c < lf.schema.size(); ++c)
        if (child[c] >= 0 && lf.schema[c].type == ColType::UTF8 && ld.cols[c].bytes + chk.add_bytes[c] >= (int64_t(1) << 31))
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan_feed: Utf8 column exceeds 2^31 bytes");
    return FLOCKGPU_OK;
}

// Room for `add_rows` more rows (`add_bytes` more bytes of a Utf8 column) behind what column c of the leaf holds: where a leaf column's buffers
// grow for an append, the ordinary feed's and the prefetched pane's device-to-device one alike.  (A column that GAINS validity in a feed is
// given the same room where apply_feed materialises it.)
static int reserve_rows(flockgpu_plan *plan, int input, size_t c, int64_t add_rows, int64_t add_bytes) {
    flockgpu_ctx *ctx = plan->ctx;
    const Leaf &lf = plan->ir.leaves[(size_t)input];
    const LeafData &ld = plan->leaves[(size_t)input];
    DevBuf &dc = plan->leaves[(size_t)input].cols[c];
    void *p = nullptr;
    if (lf.schema[c].type == ColType::UTF8) {
        FG_TRY(grow(ctx, leaf_key(plan, input, (int)c, "off"), (size_t)(ld.rows + 1) * 4, (size_t)(ld.rows + add_rows + 1) * 4 + 16, &p));
        if (!dc.offsets) FG_HIP(ctx, hipMemsetAsync(p, 0, 4, ctx->stream));
        dc.offsets = static_cast<int32_t *>(p);
        FG_TRY(grow(ctx, leaf_key(plan, input, (int)c, "bytes"), (size_t)dc.bytes, (size_t)(dc.bytes + add_bytes) + 16, &p));
    } else {
        const size_t w = col_width(lf.schema[c].type);
        FG_TRY(grow(ctx, leaf_key(plan, input, (int)c, "val"), (size_t)ld.rows * w, (size_t)(ld.rows + add_rows) * w + 16, &p));
    }
    dc.values = p;
    // a column that already carries validity keeps room for every row of the leaf: the scan fills the rows fed after the last NULL with
    // "valid" up to the leaf's row count (a batch without NULLs behind one with NULLs wrote past the validity buffer before: refused by
    // the runtime as an invalid memset, found by the rows ring's exactly-sized buffers; ADVICE r4: the prefetched pane's append had its own
    // copy of this function without the rule, and that fill ran past a validity buffer sized for the panes before)
    if (dc.valid && dc.valid_rows > 0) {
        void *vp = nullptr;
        FG_TRY(grow(ctx, leaf_key(plan, input, (int)c, "valid"), (size_t)dc.valid_rows, (size_t)(ld.rows + add_rows) + 64, &vp));
        dc.valid = static_cast<uint8_t *>(vp);
    }
    return FLOCKGPU_OK;
}

// A leaf that reads the caller's columns in place (flockgpu_plan_feed_columns, FLOCKGPU_FEED_BORROW) becomes a leaf of its own buffers with the
// same contents, so that a later feed can append: device-to-device copies on the ctx stream.  On failure the leaf stays as it was.
static int own_user_columns(flockgpu_plan *plan, int input) {
    flockgpu_ctx *ctx = plan->ctx;
    const Leaf &lf = plan->ir.leaves[(size_t)input];
    LeafData &ld = plan->leaves[(size_t)input];
    const std::vector<DevBuf> user = ld.cols;
    const int64_t rows = ld.rows;
    for (auto &c : ld.cols) c = DevBuf{};
    ld.rows = 0;
    ld.borrowed = ld.user_cols = false;
    const int rc = [&]() -> int {
        for (size_t c = 0; c < user.size(); ++c) {
            const DevBuf &u = user[c];
            if (!u.values && !u.offsets) continue;
            DevBuf &dc = ld.cols[c];
            FG_TRY(reserve_rows(plan, input, c, rows, u.bytes));
            if (lf.schema[c].type == ColType::UTF8) {
                FG_HIP(ctx, hipMemcpyAsync(dc.offsets, u.offsets, (size_t)(rows + 1) * 4, hipMemcpyDeviceToDevice, ctx->stream));   // (offsets[0] == 0: only such columns are read in place)
                if (u.bytes) FG_HIP(ctx, hipMemcpyAsync(dc.values, u.values, (size_t)u.bytes, hipMemcpyDeviceToDevice, ctx->stream));
                dc.bytes = u.bytes;
            } else if (rows) {
                FG_HIP(ctx, hipMemcpyAsync(dc.values, u.values, (size_t)rows * col_width(lf.schema[c].type), hipMemcpyDeviceToDevice, ctx->stream));
            }
            if (u.valid && u.valid_rows > 0) {
                void *vp = nullptr;
                FG_TRY(grow(ctx, leaf_key(plan, input, (int)c, "valid"), 0, (size_t)rows + 64, &vp));
                dc.valid = static_cast<uint8_t *>(vp);
                FG_HIP(ctx, hipMemcpyAsync(dc.valid, u.valid, (size_t)u.valid_rows, hipMemcpyDeviceToDevice, ctx->stream));
                dc.valid_rows = u.valid_rows;
            }
        }
        return FLOCKGPU_OK;
    }();
    if (rc != FLOCKGPU_OK) {
        ld.cols = user;
        ld.borrowed = ld.user_cols = true;
        ld.rows = rows;
        return rc;
    }
    ld.rows = rows;
    plan->col_stats.clear();
    return FLOCKGPU_OK;
}

// feed_data_sources for one leaf, second half: the checked batches are appended behind the rows the leaf holds NOW.
static int apply_feed(flockgpu_plan *plan, int input, const FeedCheck &chk, const struct ArrowArray *const *batches) {
    flockgpu_ctx *ctx = plan->ctx;
    const Leaf &lf = plan->ir.leaves[(size_t)input];
    LeafData &ld = plan->leaves[(size_t)input];
    const std::vector<int> &child = chk.child;
    const int n_batches = (int)chk.keep.size();
    plan->has_retained = false;
    plan->col_stats.clear();
    plan->scheme_state = chk.scheme_state;
    plan->scheme_tag = chk.scheme_tag;
    for (size_t c = 0; c < lf.schema.size(); ++c)
        if (child[c] >= 0) FG_TRY(reserve_rows(plan, input, c, chk.add_rows, chk.add_bytes[c]));
    const int64_t rows_end = ld.rows + chk.add_rows;   // the leaf's rows once this feed is in
    std::vector<uint8_t> tmp_vals, tmp_bytes;
    std::vector<int32_t> tmp_off;
    struct Rebase { int32_t *data; int64_t n; int32_t delta; };
    std::vector<Rebase> rebases;  // Utf8 offsets are rebased on the device once their copy is queued
    for (int b = 0; b < n_batches; ++b) {
        const ArrowArray *rb = batches[b];
        int64_t n = rb->length;
        if (n == 0) continue;
        const bool filt = chk.filtered[(size_t)b] != 0;
        const std::vector<int64_t> &k = chk.keep[(size_t)b];
        for (size_t c = 0; c < lf.schema.size(); ++c) {
            if (child[c] < 0) continue;
            DevBuf &dc = ld.cols[c];
            const ArrowArray *a = rb->children[child[c]];
            const int64_t off = a->offset + rb->offset;
            if (chk.with_valid[(size_t)b * lf.schema.size() + c]) {   // this batch's validity bytes (of the rows that stay), behind what the column holds
                const uint8_t *bits = static_cast<const uint8_t *>(a->buffers[0]);
                std::vector<uint8_t> vb;
                if (filt) for (int64_t i : k) vb.push_back((bits[(off + i) >> 3] >> ((off + i) & 7)) & 1);
                else for (int64_t i = 0; i < n; ++i) vb.push_back((bits[(off + i) >> 3] >> ((off + i) & 7)) & 1);
                void *vp = nullptr;
                FG_TRY(grow(ctx, leaf_key(plan, input, (int)c, "valid"), (size_t)dc.valid_rows, (size_t)rows_end + 64, &vp));   // (room for every row of this feed)
                dc.valid = static_cast<uint8_t *>(vp);
                if (dc.valid_rows < ld.rows) FG_HIP(ctx, hipMemsetAsync(dc.valid + dc.valid_rows, 1, (size_t)(ld.rows - dc.valid_rows), ctx->stream));
                FG_TRY(h2d(plan, dc.valid + ld.rows, vb.data(), vb.size()));
                FG_TRY(flush_jobs(plan));   // (the bytes live in a temporary)
                dc.valid_rows = ld.rows + (int64_t)vb.size();
            }
            if (lf.schema[c].type == ColType::UTF8) {
                const int32_t *so = static_cast<const int32_t *>(a->buffers[1]) + off;
                const uint8_t *src = static_cast<const uint8_t *>(a->buffers[2]);
                int64_t b0 = so[0], nbytes = (int64_t)so[n] - b0, rows_in = n;
                if (filt) {  // the surviving rows, compacted on the host (small: the outputs of aggregate stages)
                    tmp_off.assign(1, 0);
                    tmp_bytes.clear();
                    for (int64_t i : k) {
                        tmp_bytes.insert(tmp_bytes.end(), src + so[i], src + so[i + 1]);
                        tmp_off.push_back((int32_t)tmp_bytes.size());
                    }
                    so = tmp_off.data();
                    src = tmp_bytes.data();
                    b0 = 0;
                    nbytes = (int64_t)tmp_bytes.size();
                    rows_in = (int64_t)k.size();
                }
                // offsets[rows + 1 .. rows + n] = source offsets rebased onto the column's byte cursor, on the device
                FG_TRY(h2d(plan, dc.offsets + ld.rows + 1, so + 1, (size_t)rows_in * 4));
                rebases.push_back(Rebase{dc.offsets + ld.rows + 1, rows_in, (int32_t)(dc.bytes - b0)});
                if (nbytes) FG_TRY(h2d(plan, static_cast<uint8_t *>(dc.values) + dc.bytes, src + b0, (size_t)nbytes));
                if (filt) FG_TRY(flush_jobs(plan));  // the compacted copies live in temporaries that the next column reuses
                dc.bytes += nbytes;
            } else {
                const size_t w = col_width(lf.schema[c].type);
                const uint8_t *src = static_cast<const uint8_t *>(a->buffers[1]) + (size_t)off * w;
                int64_t rows_in = n;
                if (filt) {
                    tmp_vals.resize(k.size() * w);
                    for (size_t i = 0; i < k.size(); ++i) std::memcpy(tmp_vals.data() + i * w, src + (size_t)k[i] * w, w);
                    src = tmp_vals.data();
                    rows_in = (int64_t)k.size();
                }
                FG_TRY(h2d(plan, static_cast<uint8_t *>(dc.values) + (size_t)ld.rows * w, src, (size_t)rows_in * w));
                if (filt) FG_TRY(flush_jobs(plan));
            }
        }
        ld.rows += filt ? (int64_t)k.size() : n;
        if (filt) ld.dropped += n - (int64_t)k.size();
    }
    FG_TRY(flush_jobs(plan));  // every pageable buffer of this feed, several staging lanes side by side
    for (auto &r : rebases) FG_TRY(add_i32(ctx, r.data, r.n, r.delta));  // (stream-ordered behind the copies above)
    return FLOCKGPU_OK;  // no host wait: the copies are ordered before the plan's kernels on the ctx stream
}

int flockgpu_plan_feed(flockgpu_plan *plan, int input, const struct ArrowSchema *schema, const struct ArrowArray *const *batches,
                       int n_batches) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    if (plan->ring_ppw) return fail(plan->ctx, FLOCKGPU_ERR_INVALID, "plan_feed: the plan has an open pane ring (flockgpu_plan_feed_pane, or flockgpu_plan_ring_close first)");
    // (a leaf that reads the caller's device columns in place -- FLOCKGPU_FEED_BORROW -- gets its own copy of them first: feeds append)
    if (input >= 0 && input < (int)plan->leaves.size() && plan->leaves[(size_t)input].user_cols && !plan->async_pending) FG_TRY(own_user_columns(plan, input));
    FeedCheck chk;
    FG_TRY(check_feed(plan, input, schema, batches, n_batches, chk));
    return apply_feed(plan, input, chk, batches);
}

// ------------------------------------------------------------------ pane ring
// Drops the oldest pane: the rows (bytes) of the panes that stay move to the front of a second buffer, which then trades places
// with the first (source and destination of one hipMemcpyAsync must not overlap); q5's group arrays likewise.
// The retained tail of a leaf buffer moves to the front of the buffer's twin, and the two swap names.  The twin is asked for the KEPT bytes
// only: what the next pane adds is the feed's business (grow), so in the steady state both twins have reached the size two panes need and
// nothing is allocated.  (Asking for the current buffer's capacity made every window reallocate: the arena over-allocates by an eighth when
// it grows, so each twin was always an eighth smaller than the other -- 0.39 ms of hipFree + hipMalloc per window, growing without bound.)
// (min_bytes: room the twin must have beyond what is kept -- a validity column is written up to the leaf's row count when it is scanned)
static int ring_swap_in(flockgpu_ctx *ctx, const std::string &key, const void *src, size_t keep_bytes, size_t min_bytes, void **out) {
    const std::string alt = key + ".alt";
    void *p = nullptr;
    FG_TRY(arena_get(ctx, alt.c_str(), std::max<size_t>(std::max(keep_bytes, min_bytes), 64), &p));
    if (keep_bytes) FG_HIP(ctx, hipMemcpyAsync(p, src, keep_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    std::swap(ctx->arena[key], ctx->arena[alt]);
    *out = p;
    return FLOCKGPU_OK;
}
static int ring_drop_oldest(flockgpu_plan *plan) {
    flockgpu_ctx *ctx = plan->ctx;
    if (plan->ring_n == 0) return FLOCKGPU_OK;
    API_CLOCK("ring_drop_oldest");
    if (plan->ring_q5) {
        const int64_t d = plan->ring_groups.empty() ? 0 : plan->ring_groups[0];
        int64_t total = 0;
        for (int64_t g : plan->ring_groups) total += g;
        if (d && total > d) {
            void *a = nullptr, *c = nullptr;
            FG_TRY(ring_swap_in(ctx, leaf_key(plan, 0, 0, "ring.q5a"), plan->ring_auction + d, (size_t)(total - d) * 4, 0, &a));
            FG_TRY(ring_swap_in(ctx, leaf_key(plan, 0, 0, "ring.q5c"), plan->ring_count + d, (size_t)(total - d) * 4, 0, &c));
            plan->ring_auction = static_cast<int32_t *>(a);
            plan->ring_count = static_cast<uint32_t *>(c);
        }
        if (!plan->ring_groups.empty()) plan->ring_groups.erase(plan->ring_groups.begin());
    }
    for (size_t l = 0; l < plan->leaves.size(); ++l) {
        LeafData &ld = plan->leaves[l];
        const Leaf &lf = plan->ir.leaves[l];
        // (q5's state ring: the leaf holds the newest pane's rows only -- one entry, dropped only when that pane is the oldest, too)
        if (ld.pane_rows.empty() || (plan->ring_q5 && plan->ring_n > 1)) continue;
        const int64_t d = ld.pane_rows[0], keep = ld.rows - d;
        for (size_t c = 0; c < ld.cols.size(); ++c) {
            DevBuf &dc = ld.cols[c];
            if (!dc.values) continue;
            if (dc.valid && dc.valid_rows > 0) {   // the validity bytes of the rows that stay (rows beyond valid_rows are valid by convention)
                const int64_t left = std::max<int64_t>(dc.valid_rows - d, 0);
                if (left > 0 && d > 0) {
                    void *nv = nullptr;
                    FG_TRY(ring_swap_in(ctx, leaf_key(plan, (int)l, (int)c, "valid"), dc.valid + d, (size_t)left, (size_t)keep + 64, &nv));
                    dc.valid = static_cast<uint8_t *>(nv);
                }
                dc.valid_rows = left;
            }
            if (lf.schema[c].type == ColType::UTF8) {
                const int64_t db = ld.pane_bytes[0][c];
                if (keep > 0 && d > 0) {
                    void *no = nullptr, *nb = nullptr;
                    FG_TRY(ring_swap_in(ctx, leaf_key(plan, (int)l, (int)c, "off"), dc.offsets + d, (size_t)(keep + 1) * 4, 0, &no));
                    FG_TRY(ring_swap_in(ctx, leaf_key(plan, (int)l, (int)c, "bytes"), static_cast<uint8_t *>(dc.values) + db, (size_t)(dc.bytes - db), 0, &nb));
                    dc.offsets = static_cast<int32_t *>(no);
                    dc.values = nb;
                    if (db) FG_TRY(add_i32(ctx, dc.offsets, keep + 1, (int32_t)-db));
                } else if (keep == 0 && dc.offsets) {
                    FG_HIP(ctx, hipMemsetAsync(dc.offsets, 0, 4, ctx->stream));
                }
                dc.bytes -= db;
            } else if (keep > 0 && d > 0) {
                const size_t w = col_width(lf.schema[c].type);
                void *nv = nullptr;
                FG_TRY(ring_swap_in(ctx, leaf_key(plan, (int)l, (int)c, "val"), static_cast<uint8_t *>(dc.values) + (size_t)d * w, (size_t)keep * w, 0, &nv));
                dc.values = nv;
            }
        }
        ld.rows = keep;
        ld.pane_rows.erase(ld.pane_rows.begin());
        ld.pane_bytes.erase(ld.pane_bytes.begin());
    }
    plan->ring_first += 1;
    plan->ring_n -= 1;
    if (plan->ring_n == 0) plan->ring_newest_done = false;
    return FLOCKGPU_OK;
}

// q5's state ring: the newest pane's Partial aggregate -- HashAggregateExec(Partial) COUNT GROUP BY auction over the pane's rows,
// counted ONCE -- appended to the retained groups.
int flockgpu::ring_q5_partial(flockgpu_plan *plan) {
    flockgpu_ctx *ctx = plan->ctx;
    if (plan->ring_newest_done || plan->ring_n == 0) return FLOCKGPU_OK;
    API_CLOCK("ring_q5_partial");
    // the bids sit in whichever of the plan's two `bid` leaves was fed (both scan the same relation)
    const LeafData *ld = nullptr;
    int col = -1;
    for (size_t l = 0; l < plan->leaves.size() && !ld; ++l)
        for (size_t c = 0; c < plan->ir.leaves[l].schema.size(); ++c)
            if (plan->ir.leaves[l].needed[c] && plan->ir.leaves[l].schema[c].type == ColType::I32 && plan->leaves[l].rows > 0 && plan->leaves[l].cols[c].values) {
                ld = &plan->leaves[l];
                col = (int)c;
                break;
            }
    int64_t before = 0;
    for (size_t i = 0; i + 1 < plan->ring_groups.size(); ++i) before += plan->ring_groups[i];
    int64_t groups = 0;
    if (ld) {
        int64_t off[2] = {0, ld->rows};
        int32_t lo[1] = {0}, hi[1] = {1};
        flockgpu_bid_cols bc{static_cast<const int32_t *>(ld->cols[(size_t)col].values), nullptr, nullptr, nullptr, ld->rows};
        flockgpu_windows w{off, 1, lo, hi, 1};
        // The Partial stage per 8192-row TILE (q5.hip: q5_partial_tile_kernel -- one pass, one wait; a tile stands for one input partition
        // of HashAggregateExec(Partial), so an auction may leave the pane in several (auction, count) groups, which the Final side merges).
        // Going through flockgpu_q5_partial_counts instead made every window TWO full q5 calls of different kinds on one ctx -- each
        // re-uploading the other's schedule and declining its speculation: 1.48 ms per window against 1.21 ms for the whole-window feed
        // (bench, round 4).
        Q5TilePartial part;
        FG_TRY(q5_partial_by_tile(ctx, &bc, &w, &part));
        groups = part.offsets[1] - part.offsets[0];
        void *a = nullptr, *c = nullptr;
        FG_TRY(grow(ctx, leaf_key(plan, 0, 0, "ring.q5a"), (size_t)before * 4, (size_t)(before + groups) * 4 + 64, &a));
        FG_TRY(grow(ctx, leaf_key(plan, 0, 0, "ring.q5c"), (size_t)before * 4, (size_t)(before + groups) * 4 + 64, &c));
        plan->ring_auction = static_cast<int32_t *>(a);
        plan->ring_count = static_cast<uint32_t *>(c);
        if (groups) {
            FG_HIP(ctx, hipMemcpyAsync(plan->ring_auction + before, part.auction + part.offsets[0], (size_t)groups * 4, hipMemcpyDeviceToDevice, ctx->stream));
            FG_HIP(ctx, hipMemcpyAsync(plan->ring_count + before, part.count + part.offsets[0], (size_t)groups * 4, hipMemcpyDeviceToDevice, ctx->stream));
        }
    }
    plan->ring_groups.back() = groups;
    plan->ring_newest_done = true;
    return FLOCKGPU_OK;
}

int flockgpu_plan_ring_open(flockgpu_plan *plan, int panes_per_window) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    flockgpu_ctx *ctx = plan->ctx;
    if (panes_per_window < 1 || panes_per_window > 4096) return fail(ctx, FLOCKGPU_ERR_INVALID, "ring_open: %d panes per window", panes_per_window);
    if (plan->ring_ppw) return fail(ctx, FLOCKGPU_ERR_INVALID, "ring_open: the plan already has an open ring");
    for (auto &ld : plan->leaves)
        if (ld.rows || ld.borrowed) return fail(ctx, FLOCKGPU_ERR_INVALID, "ring_open: the plan holds inputs (flockgpu_plan_reset first)");
    plan->ring_ppw = panes_per_window;
    plan->ring_first = 0;
    plan->ring_n = 0;
    plan->ring_q5 = plan->query == 5 && !plan->generic_only;
    plan->ring_groups.clear();
    plan->ring_newest_done = false;
    return FLOCKGPU_OK;
}

int flockgpu_plan_ring_state(const flockgpu_plan *plan, int64_t *first_pane, int *n_panes, int *panes_per_window) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    if (first_pane) *first_pane = plan->ring_first;
    if (n_panes) *n_panes = plan->ring_n;
    if (panes_per_window) *panes_per_window = plan->ring_ppw;
    return FLOCKGPU_OK;
}

// Ends a prefetch's host side: the staging threads are joined (every copy is queued on the copy stream by then).  Returns their status.
static int prefetch_join(flockgpu_plan *plan) {
    int rc = FLOCKGPU_OK;
    for (auto &w : plan->pre.workers)
        if (w.joinable()) w.join();
    plan->pre.workers.clear();
    for (int r : plan->pre.rc)
        if (r != FLOCKGPU_OK) rc = r;
    plan->pre.rc.clear();
    return rc;
}
// Drops a pending prefetch (ring close, reset of a plan without a ring, destroy): nothing of it reaches the leaf.
void flockgpu::prefetch_drop(flockgpu_plan *plan) {
    if (!plan->pre.active) return;
    (void)prefetch_join(plan);
    if (plan->copy_stream) (void)hipStreamSynchronize(plan->copy_stream);
    plan->pre.active = false;
}

int flockgpu_plan_prefetch_pane(flockgpu_plan *plan, int input, int64_t pane_id, const struct ArrowSchema *schema, const struct ArrowArray *const *batches,
                                int n_batches) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    flockgpu_ctx *ctx = plan->ctx;
    if (!plan->ring_ppw) return fail(ctx, FLOCKGPU_ERR_INVALID, "prefetch_pane: the plan has no open ring (flockgpu_plan_ring_open)");
    if (input < 0 || input >= (int)plan->leaves.size() || !schema || !batches || n_batches < 1) return fail(ctx, FLOCKGPU_ERR_INVALID, "prefetch_pane: bad argument");
    if (plan->pre.active) return fail(ctx, FLOCKGPU_ERR_INVALID, "prefetch_pane: pane %lld of input %d is already on its way", (long long)plan->pre.pane, plan->pre.input);
    const int64_t newest = plan->ring_first + plan->ring_n - 1;
    if (plan->ring_n > 0 && pane_id != newest + 1)
        return fail(ctx, FLOCKGPU_ERR_INVALID, "prefetch_pane: pane %lld is not the next one (the ring holds [%lld, %lld])", (long long)pane_id, (long long)plan->ring_first,
                    (long long)newest);
    const Leaf &lf = plan->ir.leaves[(size_t)input];
    if (plan->leaves[(size_t)input].borrowed) return fail(ctx, FLOCKGPU_ERR_INVALID, "prefetch_pane: input %d shares another plan's relation", input);
    FG_HIP(ctx, hipSetDevice(ctx->device));
    // what the pane holds: fixed-width columns without NULLs (anything else takes the ordinary feed, which knows how to rebase and filter)
    std::vector<int> child;
    FG_TRY(match_schema(ctx, "prefetch_pane", lf, schema, &child));
    int64_t rows = 0;
    for (int b = 0; b < n_batches; ++b) {
        if (!batches[b] || batches[b]->n_children < schema->n_children) return fail(ctx, FLOCKGPU_ERR_INVALID, "prefetch_pane: batch %d does not match the schema", b);
        rows += batches[b]->length;
    }
    for (size_t c = 0; c < lf.schema.size(); ++c) {
        if (child[c] < 0) continue;
        for (int b = 0; b < n_batches; ++b) {
            const ArrowArray *rb = batches[b];
            FG_TRY(check_column(ctx, "prefetch_pane", lf.schema[c], rb, child[c]));
            if (validity_has_nulls(rb->children[child[c]], rb->children[child[c]]->offset + rb->offset, rb->length))
                return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "prefetch_pane: column '%s' holds NULLs (feed the pane the ordinary way)", lf.schema[c].name.c_str());
        }
    }
    if (rows >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "prefetch_pane: more than 2^31 rows");
    if (!plan->copy_stream) {
        FG_HIP(ctx, hipStreamCreateWithFlags(&plan->copy_stream, hipStreamNonBlocking));
        FG_HIP(ctx, hipEventCreateWithFlags(&plan->copy_done, hipEventDisableTiming));
        FG_HIP(ctx, hipEventCreateWithFlags(&plan->append_done, hipEventDisableTiming));
    }
    // the side buffers and the pinned mirror are the previous prefetch's, too: its copies must have left the mirror (host wait: they were
    // queued a whole window ago) and its appends must have read the side buffers (device-side wait of the copy stream)
    if (plan->copy_done_set) FG_HIP(ctx, hipEventSynchronize(plan->copy_done));
    if (plan->append_done_set) FG_HIP(ctx, hipStreamWaitEvent(plan->copy_stream, plan->append_done, 0));
    // side buffers; every column's batches as runs (add_run), sent once the whole pane has been looked at: pinned sources straight to the DMA
    // engine, pageable ones through a pinned mirror filled by staging threads
    plan->pre.dev.assign(lf.schema.size(), nullptr);
    plan->pre.dev_off.assign(lf.schema.size(), nullptr);
    plan->pre.bytes.assign(lf.schema.size(), 0);
    plan->pre.rebase.clear();
    std::vector<flockgpu_plan::CopyJob> runs;
    for (size_t c = 0; c < lf.schema.size(); ++c) {
        if (child[c] < 0) continue;
        if (lf.schema[c].type == ColType::UTF8) {
            // offsets: every batch's END offsets, raw, one after the other (rebased onto the column's byte cursor when the pane is appended: a run
            // of batches that are slices of one allocation shares its delta); bytes: every batch's byte range, back to back
            int64_t total = 0;
            for (int b = 0; b < n_batches; ++b) {
                const ArrowArray *rb = batches[b], *a = rb->children[child[c]];
                if (!rb->length) continue;
                const int32_t *so = static_cast<const int32_t *>(a->buffers[1]) + a->offset + rb->offset;
                total += (int64_t)so[rb->length] - so[0];
            }
            if (total >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "prefetch_pane: Utf8 column exceeds 2^31 bytes");
            void *d_off = nullptr, *d_bytes = nullptr;
            FG_TRY(arena_get(ctx, leaf_key(plan, input, (int)c, "pre.off").c_str(), (size_t)rows * 4 + 16, &d_off));
            FG_TRY(arena_get(ctx, leaf_key(plan, input, (int)c, "pre").c_str(), (size_t)total + 16, &d_bytes));
            plan->pre.dev[c] = d_bytes;
            plan->pre.dev_off[c] = d_off;
            plan->pre.bytes[c] = total;
            int64_t row_at = 0, byte_at = 0;
            for (int b = 0; b < n_batches; ++b) {
                const ArrowArray *rb = batches[b], *a = rb->children[child[c]];
                const int64_t n = rb->length;
                if (!n) continue;
                const int32_t *so = static_cast<const int32_t *>(a->buffers[1]) + a->offset + rb->offset;
                const uint8_t *sb = static_cast<const uint8_t *>(a->buffers[2]);
                const int64_t nbytes = (int64_t)so[n] - so[0], delta = byte_at - so[0];
                if (nbytes && !sb) return fail(ctx, FLOCKGPU_ERR_INVALID, "prefetch_pane: Utf8 column '%s' without a data buffer", lf.schema[c].name.c_str());
                add_run(runs, static_cast<uint8_t *>(d_off) + (size_t)row_at * 4, so + 1, (size_t)n * 4);
                if (nbytes) add_run(runs, static_cast<uint8_t *>(d_bytes) + byte_at, sb + so[0], (size_t)nbytes);
                auto &rbs = plan->pre.rebase;
                if (!rbs.empty() && rbs.back().col == (int)c && rbs.back().delta == delta && rbs.back().row0 + rbs.back().n == row_at) rbs.back().n += n;
                else rbs.push_back(flockgpu_plan::Prefetch::Rebase{(int)c, row_at, n, delta});
                row_at += n;
                byte_at += nbytes;
            }
            continue;
        }
        const size_t w = col_width(lf.schema[c].type);
        void *d = nullptr;
        FG_TRY(arena_get(ctx, leaf_key(plan, input, (int)c, "pre").c_str(), (size_t)rows * w + 16, &d));
        plan->pre.dev[c] = d;
        size_t at = 0;
        for (int b = 0; b < n_batches; ++b) {
            const ArrowArray *rb = batches[b], *a = rb->children[child[c]];
            const size_t bytes = (size_t)rb->length * w;
            if (!bytes) continue;
            add_run(runs, static_cast<uint8_t *>(d) + at, static_cast<const uint8_t *>(a->buffers[1]) + (size_t)(a->offset + rb->offset) * w, bytes);
            at += bytes;
        }
    }
    std::vector<flockgpu_plan::CopyJob> pieces;   // pageable pieces: dst (device), src (host), bytes
    size_t pageable = 0;
    FG_TRY(issue_runs(ctx, plan->copy_stream, runs, &pieces, &pageable));
    uint8_t *mirror = nullptr;   // (before the prefetch counts as under way: a refusal here must leave nothing behind that a feed would append)
    if (!pieces.empty()) FG_TRY(pinned_get_t(ctx, leaf_key(plan, input, 0, "pre.stage").c_str(), pageable + 64, &mirror));
    plan->pre.input = input;
    plan->pre.pane = pane_id;
    plan->pre.rows = rows;
    plan->pre.active = true;
    if (pieces.empty()) return FLOCKGPU_OK;
    // (the mirror may still feed the previous prefetch's copies: they were waited for when that pane was appended -- feed_pane orders the
    // ctx stream behind the copy stream, and a host synchronises the ctx stream in every execute)
    const int n_lanes = (int)std::min<size_t>(4, pieces.size());
    auto shared = std::make_shared<std::vector<flockgpu_plan::CopyJob>>(std::move(pieces));
    plan->pre.rc.assign((size_t)n_lanes, FLOCKGPU_OK);
    const int device = ctx->device;
    hipStream_t stream = plan->copy_stream;
    for (int l = 0; l < n_lanes; ++l)
        plan->pre.workers.emplace_back([plan, shared, mirror, l, n_lanes, device, stream] {
            if (hipSetDevice(device) != hipSuccess) {
                plan->pre.rc[(size_t)l] = FLOCKGPU_ERR_HIP;
                return;
            }
            uint8_t *at = mirror;   // the pieces lie in the mirror back to back; this lane fills every n_lanes-th
            for (size_t i = 0; i < shared->size(); at += (*shared)[i++].bytes) {
                const flockgpu_plan::CopyJob &j = (*shared)[i];
                if (i % (size_t)n_lanes != (size_t)l) continue;
                std::memcpy(at, j.src, j.bytes);
                if (hipMemcpyAsync(j.dst, at, j.bytes, hipMemcpyHostToDevice, stream) != hipSuccess) plan->pre.rc[(size_t)l] = FLOCKGPU_ERR_HIP;
            }
        });
    return FLOCKGPU_OK;
}

// The ring's bookkeeping around the feed of one pane, for host batches (flockgpu_plan_feed_pane) and device columns
// (flockgpu_plan_feed_pane_columns) alike: pane_turn decides whether `pane_id` may be fed now and whether it begins a new pane (nothing changes),
// pane_begin opens that pane, pane_undo takes the opening back after a feed that failed behind its validation, pane_fed books what a feed appended.
struct PaneTurn {
    int64_t pane_id = 0;
    bool begin = false;
    // what pane_begin changes, kept so that a feed that fails AFTER its validation (allocation, HIP error, staging) leaves the rows ring as it
    // was.  q5's state ring cannot go back -- the closing pane's rows are folded into its groups by then -- so there a failed
    // first feed leaves the new pane begun and empty: the same pane id is simply fed again.
    int ring_n_before = 0;
    int64_t ring_first_before = 0;
    bool newest_done_before = false;
};
static int pane_turn(flockgpu_plan *plan, const char *who, int64_t pane_id, PaneTurn *turn) {
    flockgpu_ctx *ctx = plan->ctx;
    const int64_t newest = plan->ring_first + plan->ring_n - 1;
    const bool begin = plan->ring_n == 0 || pane_id == newest + 1;
    if (!begin && pane_id != newest)
        return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: pane %lld out of order -- the ring holds panes [%lld, %lld], only pane %lld or %lld can be fed", who,
                    (long long)pane_id, (long long)plan->ring_first, (long long)newest, (long long)newest, (long long)(newest + 1));
    if (begin && plan->ring_n == plan->ring_ppw)
        return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: the ring is full (%d panes): flockgpu_plan_reset retires the oldest before pane %lld begins", who,
                    plan->ring_ppw, (long long)pane_id);
    turn->pane_id = pane_id;
    turn->begin = begin;
    return FLOCKGPU_OK;
}
static int pane_begin(flockgpu_plan *plan, PaneTurn *turn) {
    turn->ring_n_before = plan->ring_n;
    turn->ring_first_before = plan->ring_first;
    turn->newest_done_before = plan->ring_newest_done;
    if (!turn->begin) return FLOCKGPU_OK;
    if (plan->ring_q5 && plan->ring_n > 0) {   // the pane that closes leaves its groups behind, its rows go
        FG_TRY(ring_q5_partial(plan));
        for (auto &ld : plan->leaves) {
            ld.rows = 0;
            for (auto &c : ld.cols) c.bytes = 0;
            ld.pane_rows.clear();
            ld.pane_bytes.clear();
        }
    }
    if (plan->ring_n == 0) plan->ring_first = turn->pane_id;
    plan->ring_n += 1;
    for (size_t l = 0; l < plan->leaves.size(); ++l) {
        plan->leaves[l].pane_rows.push_back(0);
        plan->leaves[l].pane_bytes.emplace_back(plan->leaves[l].cols.size(), 0);
    }
    if (plan->ring_q5) plan->ring_groups.push_back(0);
    plan->ring_newest_done = false;
    return FLOCKGPU_OK;
}
static void pane_undo(flockgpu_plan *plan, const PaneTurn &turn) {
    if (!turn.begin || plan->ring_q5) return;
    plan->ring_n = turn.ring_n_before;
    plan->ring_first = turn.ring_first_before;
    plan->ring_newest_done = turn.newest_done_before;
    for (auto &l : plan->leaves) {
        if (!l.pane_rows.empty()) l.pane_rows.pop_back();
        if (!l.pane_bytes.empty()) l.pane_bytes.pop_back();
    }
}
// The newest pane gained what `ld` holds beyond `before`.
static void pane_fed(flockgpu_plan *plan, LeafData &ld, const LeafSnapshot &before) {
    ld.pane_rows.back() += ld.rows - before.rows;
    for (size_t c = 0; c < ld.cols.size(); ++c) ld.pane_bytes.back()[c] += ld.cols[c].bytes - before.bytes[c];
    plan->ring_newest_done = false;   // (more rows of the newest pane: its groups are counted again from its rows)
    if (plan->ring_q5) plan->ring_groups.back() = 0;
}

int flockgpu_plan_feed_pane(flockgpu_plan *plan, int input, int64_t pane_id, const struct ArrowSchema *schema,
                            const struct ArrowArray *const *batches, int n_batches) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    flockgpu_ctx *ctx = plan->ctx;
    if (!plan->ring_ppw) return fail(ctx, FLOCKGPU_ERR_INVALID, "feed_pane: the plan has no open ring (flockgpu_plan_ring_open)");
    API_CLOCK("feed_pane");
    plan->col_stats.clear();
    if (input < 0 || input >= (int)plan->leaves.size()) return fail(ctx, FLOCKGPU_ERR_INVALID, "feed_pane: bad argument");
    PaneTurn turn;
    FG_TRY(pane_turn(plan, "feed_pane", pane_id, &turn));
    // a pane that flockgpu_plan_prefetch_pane already brought over: its side buffers are appended below, device to device
    const bool from_prefetch = n_batches == 0 && !schema && plan->pre.active && plan->pre.input == input && plan->pre.pane == pane_id;
    if (plan->pre.active && !from_prefetch && plan->pre.input == input)
        return fail(ctx, FLOCKGPU_ERR_INVALID, "feed_pane: pane %lld of input %d was prefetched: feed it with (NULL, NULL, 0) first", (long long)plan->pre.pane, plan->pre.input);
    if (from_prefetch) {
        const int rc_pre = prefetch_join(plan);
        if (rc_pre != FLOCKGPU_OK) {
            plan->pre.active = false;
            return fail(ctx, rc_pre, "feed_pane: the prefetch of pane %lld failed while staging", (long long)pane_id);
        }
    }
    // every check of the feed first: a refused feed must leave the ring as it was
    FeedCheck chk;
    {
        API_CLOCK2(c1, "feed_pane.validate");
        if (n_batches > 0 || schema) FG_TRY(check_feed(plan, input, schema, batches, n_batches, chk));
    }
    auto undo_begin = [&]() { pane_undo(plan, turn); };
    FG_TRY(pane_begin(plan, &turn));
    // the leaf's cursors as the pane's feed finds them: what a feed that fails half-way goes back to
    LeafData &ld = plan->leaves[(size_t)input];
    const LeafSnapshot before(ld);
    if (from_prefetch) {
      const int rc_append = [&]() -> int {
        const Leaf &lf = plan->ir.leaves[(size_t)input];
        FG_HIP(ctx, hipEventRecord(plan->copy_done, plan->copy_stream));           // every copy of the pane is queued (prefetch_join)
        plan->copy_done_set = true;
        FG_HIP(ctx, hipStreamWaitEvent(ctx->stream, plan->copy_done, 0));          // ... and the appends wait for them on the device
        for (size_t c = 0; c < lf.schema.size(); ++c) {
            if (!plan->pre.dev[c]) continue;
            DevBuf &dc = ld.cols[c];
            FG_TRY(reserve_rows(plan, input, c, plan->pre.rows, plan->pre.bytes[c]));
            if (lf.schema[c].type == ColType::UTF8) {   // offsets behind the leaf's, rebased onto its byte cursor run by run; bytes behind its bytes
                if (dc.bytes + plan->pre.bytes[c] >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "feed_pane: Utf8 column exceeds 2^31 bytes");
                if (plan->pre.rows) {
                    FG_HIP(ctx, hipMemcpyAsync(dc.offsets + ld.rows + 1, plan->pre.dev_off[c], (size_t)plan->pre.rows * 4, hipMemcpyDeviceToDevice, ctx->stream));
                    for (auto &rb : plan->pre.rebase)
                        if (rb.col == (int)c) FG_TRY(add_i32(ctx, dc.offsets + ld.rows + 1 + rb.row0, rb.n, (int32_t)(dc.bytes + rb.delta)));
                }
                if (plan->pre.bytes[c])
                    FG_HIP(ctx, hipMemcpyAsync(static_cast<uint8_t *>(dc.values) + dc.bytes, plan->pre.dev[c], (size_t)plan->pre.bytes[c], hipMemcpyDeviceToDevice, ctx->stream));
                dc.bytes += plan->pre.bytes[c];
                ld.pane_bytes.back()[c] += plan->pre.bytes[c];
                continue;
            }
            const size_t w = col_width(lf.schema[c].type);
            if (plan->pre.rows)
                FG_HIP(ctx, hipMemcpyAsync(static_cast<uint8_t *>(dc.values) + (size_t)ld.rows * w, plan->pre.dev[c], (size_t)plan->pre.rows * w, hipMemcpyDeviceToDevice, ctx->stream));
        }
        FG_HIP(ctx, hipEventRecord(plan->append_done, ctx->stream));
        plan->append_done_set = true;
        ld.rows += plan->pre.rows;
        ld.pane_rows.back() += plan->pre.rows;
        plan->has_retained = false;
        plan->fed_bytes += 1;   // (reset waits for the stream before the host's buffers may go)
        plan->pre.active = false;
        plan->ring_newest_done = false;
        if (plan->ring_q5) plan->ring_groups.back() = 0;
        return FLOCKGPU_OK;
      }();
      if (rc_append != FLOCKGPU_OK) {   // (the prefetch stays pending: the same call can be repeated)
          // a later column's failure must not leave an earlier column's byte cursor advanced: the retry would append behind the orphaned bytes
          // while offsets[ld.rows] still names the old end
          for (size_t c = 0; c < ld.cols.size(); ++c)
              if (!ld.pane_bytes.empty()) ld.pane_bytes.back()[c] -= ld.cols[c].bytes - before.bytes[c];
          before.restore(ld);
          undo_begin();
      }
      return rc_append;
    }
    if (n_batches == 0) return FLOCKGPU_OK;   // an empty pane still advances the ring
    {
        API_CLOCK2(c2, "feed_pane.feed");
        const int rc_feed = apply_feed(plan, input, chk, batches);
        if (rc_feed != FLOCKGPU_OK) {
            // (rows of batches that did get through stay appended to the leaf's buffers but are not counted: ld.rows is what the ring reads)
            if (!plan->ring_q5) before.restore(ld);
            undo_begin();
            return rc_feed;
        }
    }
    pane_fed(plan, ld, before);
    return FLOCKGPU_OK;
}

int flockgpu_plan_ring_close(flockgpu_plan *plan) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    if (plan->async_pending) return fail(plan->ctx, FLOCKGPU_ERR_INVALID, "ring_close: an asynchronous execute is in flight");
    prefetch_drop(plan);
#ifdef FLOCKGPU_EXPERIMENTAL
    ApiClock::dump();
#endif
    plan->ring_ppw = 0;
    plan->ring_n = 0;
    plan->ring_q5 = false;
    plan->ring_groups.clear();
    plan->ring_newest_done = false;
    return flockgpu_plan_reset(plan);
}

int flockgpu_plan_reset(flockgpu_plan *plan) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    if (plan->async_pending) return fail(plan->ctx, FLOCKGPU_ERR_INVALID, "plan_reset: an asynchronous execute is in flight (flockgpu_plan_wait first)");
    plan->col_stats.clear();
    API_CLOCK("reset");
    // borrowed pinned buffers may still be read by the DMA engine: the caller is about to drop them
    if (plan->fed_bytes || plan->device_fed) (void)hipStreamSynchronize(plan->ctx->stream);
    plan->fed_bytes = 0;
    plan->device_fed = false;
    plan->has_retained = false;   // (its columns may alias the leaves, and the arena buffers behind it are reused by the next execute)
    plan->scheme_state = -1;
    plan->scheme_tag.clear();
    if (plan->ring_ppw) {   // the window ends: the oldest pane of a full ring goes, the others stay on the device
        if (plan->ring_n == plan->ring_ppw) FG_TRY(ring_drop_oldest(plan));
        return FLOCKGPU_OK;
    }
    for (auto &ld : plan->leaves) {
        ld.rows = 0;
        ld.dropped = 0;
        ld.pane_rows.clear();
        ld.pane_bytes.clear();
        for (auto &c : ld.cols) {
            c.bytes = 0;
            c.valid_rows = 0;
            if (ld.borrowed) c.values = nullptr, c.offsets = nullptr, c.valid = nullptr;   // the donor's memory: never grown or appended to from here
        }
        ld.borrowed = false;
        ld.user_cols = false;
    }
    return FLOCKGPU_OK;
}

// The column of `have` that a leaf column `want` can read in place: same name, same type (the last such; -1: none).  `held`: the columns of
// `have` that carry data (null: all of them).
static int find_field(const std::vector<Field> &have, const std::vector<char> *held, const Field &want) {
    int at = -1;
    for (size_t d = 0; d < have.size(); ++d)
        if ((!held || (*held)[d]) && have[d].name == want.name && have[d].type == want.type) at = (int)d;
    return at;
}

int flockgpu_plan_feed_shared(flockgpu_plan *plan, int input, const flockgpu_plan *donor, int donor_input) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    flockgpu_ctx *ctx = plan->ctx;
    if (!donor || donor == plan || input < 0 || input >= (int)plan->ir.leaves.size() || donor_input < 0 || donor_input >= (int)donor->ir.leaves.size())
        return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed_shared: bad argument");
    if (donor->ctx != ctx) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed_shared: the two plans live on different contexts (streams)");
    if (plan->ring_ppw || donor->ring_ppw) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed_shared: a plan with an open pane ring feeds panes (flockgpu_plan_feed_pane)");
    const Leaf &lf = plan->ir.leaves[(size_t)input], &df = donor->ir.leaves[(size_t)donor_input];
    LeafData &ld = plan->leaves[(size_t)input];
    const LeafData &dd = donor->leaves[(size_t)donor_input];
    if (ld.rows != 0 || ld.borrowed) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed_shared: input %d already holds rows", input);
    if (dd.borrowed) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed_shared: the donor's relation is itself shared");
    // what the donor left out because of NULLs it was allowed to drop need not be droppable here
    if (dd.dropped) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan_feed_shared: the donor dropped %lld rows with NULLs", (long long)dd.dropped);
    std::vector<int> from(lf.schema.size(), -1);
    for (size_t c = 0; c < lf.schema.size(); ++c) {
        if (!lf.needed[c]) continue;
        from[c] = find_field(df.schema, &df.needed, lf.schema[c]);
        if (from[c] < 0)
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan_feed_shared: the donor does not hold column '%s' as %s", lf.schema[c].name.c_str(), type_name(lf.schema[c]));
        if (dd.rows > 0 && !dd.cols[(size_t)from[c]].values) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed_shared: the donor has not been fed");
    }
    for (size_t c = 0; c < lf.schema.size(); ++c)
        if (from[c] >= 0) ld.cols[c] = dd.cols[(size_t)from[c]];
    ld.rows = dd.rows;
    ld.borrowed = true;
    return FLOCKGPU_OK;   // same stream as the donor's copies: ordered behind them without a wait
}

int flockgpu_plan_feed_from(flockgpu_plan *plan, int input, const flockgpu_plan *producer) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    flockgpu_ctx *ctx = plan->ctx;
    if (!producer || producer == plan || input < 0 || input >= (int)plan->ir.leaves.size()) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed_from: bad argument");
    if (producer->ctx != ctx) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed_from: the two plans live on different contexts (streams)");
    if (plan->ring_ppw) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed_from: a plan with an open pane ring feeds panes (flockgpu_plan_feed_pane)");
    if (!producer->has_retained) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed_from: the producer holds no retained result (flockgpu_plan_execute_retain)");
    const Leaf &lf = plan->ir.leaves[(size_t)input];
    LeafData &ld = plan->leaves[(size_t)input];
    if (ld.rows != 0 || ld.borrowed) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed_from: input %d already holds rows", input);
    const std::vector<Field> &ps = producer->ir.root->schema;
    const Table &t = producer->retained;
    std::vector<int> from(lf.schema.size(), -1);
    bool empty = false;   // a NULL the plan may drop (MAX over no rows): the relation is empty
    for (size_t c = 0; c < lf.schema.size(); ++c) {
        if (!lf.needed[c]) continue;
        from[c] = find_field(ps, nullptr, lf.schema[c]);
        if (from[c] < 0) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan_feed_from: the producer's result has no column '%s' of type %s", lf.schema[c].name.c_str(), type_name(lf.schema[c]));
        if (t.cols[(size_t)from[c]].c.all_null) {
            if (!lf.null_droppable[c]) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "plan_feed_from: column '%s' is NULL and would reach the output", lf.schema[c].name.c_str());
            empty = true;
        }
    }
    if (empty || t.rows == 0) return FLOCKGPU_OK;   // an unfed leaf is an empty relation
    for (size_t c = 0; c < lf.schema.size(); ++c) {
        if (from[c] < 0) continue;
        const DevColumn &col = t.cols[(size_t)from[c]].c;
        ld.cols[c] = DevBuf{const_cast<void *>(col.values), const_cast<int32_t *>(col.offsets), col.bytes, const_cast<uint8_t *>(col.valid), col.valid ? t.rows : 0};
    }
    ld.rows = t.rows;
    ld.borrowed = true;
    return FLOCKGPU_OK;
}

// ------------------------------------------------------------------ device columns in and out (flockgpu_plan_feed_columns / _result_columns)
namespace {

// The Arrow format a FLOCKGPU_TEXT_* type stands for (the refusals speak the host feed's language).
const char *text_format(int32_t t) {
    switch (t) {
        case FLOCKGPU_TEXT_INT32: return "i";
        case FLOCKGPU_TEXT_INT64: return "l";
        case FLOCKGPU_TEXT_UINT64: return "L";
        case FLOCKGPU_TEXT_FLOAT64: return "g";
        case FLOCKGPU_TEXT_TIMESTAMP_MS: return "tsm:";
        case FLOCKGPU_TEXT_UTF8: return "u";
        default: return "?";
    }
}
int32_t text_type_of(const Field &f) {
    if (f.is_ts) return FLOCKGPU_TEXT_TIMESTAMP_MS;
    switch (f.type) {
        case ColType::I32: return FLOCKGPU_TEXT_INT32;
        case ColType::I64: return FLOCKGPU_TEXT_INT64;
        case ColType::U64: return FLOCKGPU_TEXT_UINT64;
        case ColType::F64: return FLOCKGPU_TEXT_FLOAT64;
        default: return FLOCKGPU_TEXT_UTF8;
    }
}
bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

// What columns_check found out about a feed of device columns and columns_apply acts on (FeedCheck's twin; the two halves of
// flockgpu_plan_feed_columns, which flockgpu_plan_feed_pane_columns runs either side of the ring's begin).
struct ColumnsCheck {
    bool nothing = false;                     // no rows: the feed is a no-op
    std::vector<int> at, utf8_of;             // leaf column -> fed column (-1: not read) / its Utf8 slot in the census (-1: fixed width)
    std::vector<char> with_valid;             // NULLs that stay -> validity bytes go along
    std::vector<int64_t> first, add_bytes;    // per Utf8 column: its first byte in the source, the bytes it adds
    std::vector<flockgpu_utf8> taken;         // per Utf8 column: the surviving rows, when rows are left out
    const int32_t *keep_rows = nullptr;       // the rows that stay, when rows are left out
    bool drop = false;
    int64_t n_keep = 0;
    int scheme_state = -1;
};

// Device columns for one leaf, first half: every check of the feed -- the match by name, the census of NULLs and Utf8 byte ranges, the take of the
// Utf8 survivors -- with nothing of the plan or the leaf changed.  `who` begins the messages.
static int columns_check(flockgpu_plan *plan, int input, const flockgpu_text_column *cols, int32_t n_cols, int64_t rows, const char *who, ColumnsCheck &ck) {
    flockgpu_ctx *ctx = plan->ctx;
    ck.nothing = false;
    if (plan->async_pending) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: an asynchronous execute is in flight (flockgpu_plan_wait first)", who);
    FG_HIP(ctx, hipSetDevice(ctx->device));
    const Leaf &lf = plan->ir.leaves[(size_t)input];
    LeafData &ld = plan->leaves[(size_t)input];
    if (ld.borrowed && !ld.user_cols) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: input %d shares another plan's relation; reset the plan first", who, input);
    // hash placement: device columns carry no scheme tag -- an untagged batch
    int &scheme_state = ck.scheme_state;
    scheme_state = plan->scheme_state;
    if (lf.co_partitioned && rows > 0) {
        if (scheme_state == 1)
            return fail(ctx, FLOCKGPU_ERR_INVALID,
                        "%s: mixed hash placement -- this stage was fed partitions tagged '%s' and untagged ones (another engine's hash): "
                        "every producer of a stage must place rows the same way", who, kPartitionScheme);
        scheme_state = 0;
    }
    // the columns the leaf reads, by name (match_schema's rules and messages)
    const size_t n_leaf = lf.schema.size();
    std::vector<int> &at = ck.at;
    at.assign(n_leaf, -1);
    for (size_t c = 0; c < n_leaf; ++c) {
        if (!lf.needed[c]) continue;
        for (int32_t i = 0; i < n_cols && at[c] < 0; ++i)
            if (cols[i].name && lf.schema[c].name == cols[i].name) at[c] = i;
        if (at[c] < 0) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: column '%s' missing from the fed schema", who, lf.schema[c].name.c_str());
        const flockgpu_text_column &col = cols[at[c]];
        if (!format_ok(lf.schema[c], text_format(col.type)))
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: column '%s' has Arrow format '%s', the plan scans %s", who, lf.schema[c].name.c_str(), text_format(col.type),
                        type_name(lf.schema[c]));
    }
    // (before anything is allocated or launched)
    if (rows >= (int64_t(1) << 31) || ld.rows + rows >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than 2^31 rows per relation", who);
    if (rows == 0) {
        ck.nothing = true;
        return FLOCKGPU_OK;
    }
    CensusArgs ca;
    std::vector<int> census_of(n_leaf, -1);
    std::vector<int> &utf8_of = ck.utf8_of;
    utf8_of.assign(n_leaf, -1);
    for (size_t c = 0; c < n_leaf; ++c) {
        if (at[c] < 0) continue;
        const flockgpu_text_column &col = cols[at[c]];
        const bool utf8 = lf.schema[c].type == ColType::UTF8;
        if (utf8 ? !col.utf8.offsets : !col.values)
            return fail(ctx, FLOCKGPU_ERR_INVALID, utf8 ? "%s: Utf8 column '%s' without offsets" : "%s: column '%s' without a data buffer", who, lf.schema[c].name.c_str());
        if (!aligned_to(utf8 ? (const void *)col.utf8.offsets : col.values, utf8 ? 4 : col_width(lf.schema[c].type)))
            return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: column '%s' is not aligned to its element size", who, lf.schema[c].name.c_str());
        if (col.valid) {
            if (ca.n_valid == kCensusCols) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than %d columns with validity bytes", who, kCensusCols);
            if (lf.null_droppable[c]) ca.droppable |= uint64_t(1) << ca.n_valid;
            ca.valid[ca.n_valid] = col.valid;
            census_of[c] = ca.n_valid++;
        }
        if (utf8) {
            if (ca.n_utf8 == kCensusUtf8) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than %d Utf8 columns", who, kCensusUtf8);
            ca.offsets[ca.n_utf8] = col.utf8.offsets;
            utf8_of[c] = ca.n_utf8++;
        }
    }
    // ---- census: NULLs per column, the rows that stay, the Utf8 columns' byte ranges -- one launch, one wait (none without validity and Utf8)
    const std::string base = leaf_key(plan, input, 0, "src");
    CensusResult cr;
    FG_TRY(feed_census_begin(ctx, base.c_str(), ca, rows, &cr));
    FG_TRY(feed_census_wait(ctx, cr));
    bool &drop = ck.drop;
    drop = false;
    std::vector<char> &with_valid = ck.with_valid;
    with_valid.assign(n_leaf, 0);
    for (size_t c = 0; c < n_leaf; ++c) {
        if (census_of[c] < 0 || cr.nulls(census_of[c]) == 0) continue;   // (validity bytes that are all 1 do not reach the leaf)
        if (lf.null_droppable[c]) drop = true;
        else if (plan->ring_ppw && plan->ring_q5)   // (check_feed's refusal: q5's ring keeps Partial COUNT groups of plain columns)
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: column '%s' holds NULLs that reach the output; q5's pane ring keeps no validity", who, lf.schema[c].name.c_str());
        else with_valid[c] = 1;
    }
    int64_t &n_keep = ck.n_keep;
    n_keep = drop ? cr.kept() : rows;
    std::vector<int64_t> &first = ck.first, &add_bytes = ck.add_bytes;
    first.assign(n_leaf, 0);
    add_bytes.assign(n_leaf, 0);
    for (size_t c = 0; c < n_leaf; ++c) {
        if (utf8_of[c] < 0) continue;
        first[c] = cr.utf8_first(utf8_of[c]);
        add_bytes[c] = cr.utf8_last(utf8_of[c]) - first[c];
        if (first[c] < 0 || add_bytes[c] < 0) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: the offsets of Utf8 column '%s' decrease", who, lf.schema[c].name.c_str());
        if (add_bytes[c] && !cols[at[c]].utf8.data) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: Utf8 column '%s' without a data buffer", who, lf.schema[c].name.c_str());
    }
    // ---- rows with NULLs that may be left out: the row list, and the Utf8 columns taken at it (their byte totals: the take's own wait)
    const int32_t *&keep_rows = ck.keep_rows;
    keep_rows = nullptr;
    std::vector<flockgpu_utf8> &taken = ck.taken;
    taken.assign(n_leaf, flockgpu_utf8{nullptr, nullptr});
    if (drop && n_keep > 0) {
        FG_TRY(feed_census_rows(ctx, base.c_str(), cr, rows, n_keep, &keep_rows));
        std::vector<size_t> u8;
        for (size_t c = 0; c < n_leaf; ++c)
            if (utf8_of[c] >= 0) u8.push_back(c);
        for (size_t g0 = 0; g0 < u8.size(); g0 += 4) {
            const int k = (int)std::min<size_t>(4, u8.size() - g0);
            flockgpu_utf8 srcs[4], outs[4];
            int64_t nb[4] = {0, 0, 0, 0};
            for (int j = 0; j < k; ++j) srcs[j] = cols[at[u8[g0 + (size_t)j]]].utf8;
            Utf8MultiGather g;
            FG_TRY(gather_utf8_multi_begin(ctx, (base + ".take" + std::to_string(g0)).c_str(), srcs, k, keep_rows, n_keep, &g));
            FG_TRY(gather_utf8_multi_wait(ctx, g));
            FG_TRY(gather_utf8_multi_finish(ctx, g, outs, nb));
            for (int j = 0; j < k; ++j) {
                taken[u8[g0 + (size_t)j]] = outs[j];
                add_bytes[u8[g0 + (size_t)j]] = nb[j];
            }
        }
    } else if (drop) {
        for (size_t c = 0; c < n_leaf; ++c) add_bytes[c] = 0;
    }
    for (size_t c = 0; c < n_leaf; ++c)
        if (utf8_of[c] >= 0 && ld.cols[c].bytes + add_bytes[c] >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: Utf8 column exceeds 2^31 bytes", who);
    // (rows behind columns that are read in place: the leaf gets its own copy of those first -- before anything of the plan's state changes, so that
    // a failure here leaves plan and leaf as they were)
    if (n_keep > 0 && ld.user_cols) FG_TRY(own_user_columns(plan, input));
    return FLOCKGPU_OK;
}

// Device columns for one leaf, second half: the checked columns are appended behind the rows the leaf holds NOW (or, FLOCKGPU_FEED_BORROW, read in
// place).  A failure leaves the leaf's cursors where they were.
static int columns_apply(flockgpu_plan *plan, int input, const flockgpu_text_column *cols, int64_t rows, uint32_t flags, const ColumnsCheck &ck) {
    flockgpu_ctx *ctx = plan->ctx;
    const Leaf &lf = plan->ir.leaves[(size_t)input];
    LeafData &ld = plan->leaves[(size_t)input];
    const size_t n_leaf = lf.schema.size();
    const std::vector<int> &at = ck.at, &utf8_of = ck.utf8_of;
    const std::vector<char> &with_valid = ck.with_valid;
    const std::vector<int64_t> &first = ck.first, &add_bytes = ck.add_bytes;
    const std::vector<flockgpu_utf8> &taken = ck.taken;
    const int32_t *keep_rows = ck.keep_rows;
    const bool drop = ck.drop;
    const int64_t n_keep = ck.n_keep;
    const int scheme_state = ck.scheme_state;
    // ---- every check is behind us: from here on the leaf changes (apply_feed's resets)
    plan->has_retained = false;
    plan->col_stats.clear();
    plan->scheme_state = scheme_state;
    if (scheme_state == 0) plan->scheme_tag.clear();
    plan->device_fed = true;   // (reset waits for the stream before the caller's columns may go)
    if (n_keep == 0) {
        ld.dropped += rows;
        return FLOCKGPU_OK;
    }
    // ---- in place, when the caller lends the columns and nothing has to move
    if ((flags & FLOCKGPU_FEED_BORROW) && ld.rows == 0 && !ld.borrowed && !drop) {
        bool ok = true;
        for (size_t c = 0; c < n_leaf && ok; ++c) {
            if (at[c] < 0) continue;
            const flockgpu_text_column &col = cols[at[c]];
            if (utf8_of[c] >= 0) ok = first[c] == 0 && col.utf8.data && aligned_to(col.utf8.offsets, 16) && aligned_to(col.utf8.data, 16);
            else ok = aligned_to(col.values, 16);
            if (with_valid[c]) ok = ok && aligned_to(col.valid, 4);   // (the evaluator reads validity bytes four at a time)
        }
        if (ok) {
            for (size_t c = 0; c < n_leaf; ++c) {
                if (at[c] < 0) continue;
                const flockgpu_text_column &col = cols[at[c]];
                const bool utf8 = utf8_of[c] >= 0;
                ld.cols[c] = DevBuf{const_cast<void *>(utf8 ? (const void *)col.utf8.data : col.values), utf8 ? const_cast<int32_t *>(col.utf8.offsets) : nullptr,
                                    utf8 ? add_bytes[c] : 0, with_valid[c] ? const_cast<uint8_t *>(col.valid) : nullptr, with_valid[c] ? rows : 0};
            }
            ld.rows = rows;
            ld.borrowed = ld.user_cols = true;
            return FLOCKGPU_OK;
        }
    }
    // ---- append behind what the leaf holds
    const LeafSnapshot before(ld);
    const int rc = [&]() -> int {
        for (size_t c = 0; c < n_leaf; ++c)
            if (at[c] >= 0) FG_TRY(reserve_rows(plan, input, c, n_keep, add_bytes[c]));
        const int64_t rows_end = ld.rows + n_keep;
        TailTakeCols tk;
        auto take = [&](const void *src, void *out, int32_t width) -> int {
            tk.src[tk.n] = src;
            tk.out[tk.n] = out;
            tk.width[tk.n] = width;
            if (++tk.n < kGatherMulti) return FLOCKGPU_OK;
            const int rc_take = take_to_tail(ctx, tk, keep_rows, n_keep);
            tk.n = 0;
            return rc_take;
        };
        for (size_t c = 0; c < n_leaf; ++c) {
            if (at[c] < 0) continue;
            const flockgpu_text_column &col = cols[at[c]];
            DevBuf &dc = ld.cols[c];
            if (with_valid[c]) {   // this feed's validity bytes (of the rows that stay) behind what the column holds; the rows before, if they had none: valid
                void *vp = nullptr;
                FG_TRY(grow(ctx, leaf_key(plan, input, (int)c, "valid"), (size_t)dc.valid_rows, (size_t)rows_end + 64, &vp));
                dc.valid = static_cast<uint8_t *>(vp);
                if (dc.valid_rows < ld.rows) FG_HIP(ctx, hipMemsetAsync(dc.valid + dc.valid_rows, 1, (size_t)(ld.rows - dc.valid_rows), ctx->stream));
                if (drop) FG_TRY(take(col.valid, dc.valid + ld.rows, 1));
                else FG_HIP(ctx, hipMemcpyAsync(dc.valid + ld.rows, col.valid, (size_t)rows, hipMemcpyDeviceToDevice, ctx->stream));
                dc.valid_rows = rows_end;
            }
            if (utf8_of[c] >= 0) {   // offsets land rebased onto the column's byte cursor; only the bytes the offsets name are copied
                const int32_t *so = drop ? taken[c].offsets : col.utf8.offsets;
                const uint8_t *sb = drop ? taken[c].data : col.utf8.data + first[c];
                FG_TRY(append_offsets_rebased(ctx, dc.offsets + ld.rows + 1, so, n_keep, (int32_t)dc.bytes));
                if (add_bytes[c]) FG_HIP(ctx, hipMemcpyAsync(static_cast<uint8_t *>(dc.values) + dc.bytes, sb, (size_t)add_bytes[c], hipMemcpyDeviceToDevice, ctx->stream));
                dc.bytes += add_bytes[c];
            } else {
                const size_t w = col_width(lf.schema[c].type);
                uint8_t *dst = static_cast<uint8_t *>(dc.values) + (size_t)ld.rows * w;
                if (drop) FG_TRY(take(col.values, dst, (int32_t)w));
                else FG_HIP(ctx, hipMemcpyAsync(dst, col.values, (size_t)rows * w, hipMemcpyDeviceToDevice, ctx->stream));
            }
        }
        if (tk.n) FG_TRY(take_to_tail(ctx, tk, keep_rows, n_keep));
        return FLOCKGPU_OK;
    }();
    if (rc != FLOCKGPU_OK) {
        before.restore(ld);
        return rc;
    }
    ld.rows += n_keep;
    ld.dropped += rows - n_keep;
    return FLOCKGPU_OK;   // the copies are ordered before the plan's kernels on the ctx stream
}

int flockgpu_plan_feed_columns(flockgpu_plan *plan, int input, const flockgpu_text_column *cols, int32_t n_cols, int64_t rows, uint32_t flags) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    flockgpu_ctx *ctx = plan->ctx;
    if (plan->ring_ppw)
        return fail(ctx, FLOCKGPU_ERR_INVALID,
                    "plan_feed_columns: the plan has an open pane ring (flockgpu_plan_feed_pane / flockgpu_plan_feed_pane_columns, or flockgpu_plan_ring_close first)");
    if (input < 0 || input >= (int)plan->ir.leaves.size() || n_cols < 0 || (n_cols && !cols) || rows < 0 || (flags & ~(uint32_t)FLOCKGPU_FEED_BORROW))
        return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_feed_columns: bad argument");
    ColumnsCheck ck;
    FG_TRY(columns_check(plan, input, cols, n_cols, rows, "plan_feed_columns", ck));
    if (ck.nothing) return FLOCKGPU_OK;
    return columns_apply(plan, input, cols, rows, flags, ck);
}

int flockgpu_plan_feed_pane_columns(flockgpu_plan *plan, int input, int64_t pane_id, const flockgpu_text_column *cols, int32_t n_cols, int64_t rows,
                                    uint32_t flags) {
    static const char *const who = "plan_feed_pane_columns";
    if (!plan) return FLOCKGPU_ERR_INVALID;
    flockgpu_ctx *ctx = plan->ctx;
    if (flags & (uint32_t)FLOCKGPU_FEED_BORROW)
        return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: FLOCKGPU_FEED_BORROW does not go with a pane: the ring outlives the reset that ends a borrow", who);
    if (flags) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: flags must be 0", who);
    if (!plan->ring_ppw) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: the plan has no open pane ring (flockgpu_plan_ring_open)", who);
    API_CLOCK("feed_pane_columns");
    if (input < 0 || input >= (int)plan->ir.leaves.size() || n_cols < 0 || (n_cols && !cols) || rows < 0 || (rows > 0 && !cols))
        return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: bad argument", who);
    PaneTurn turn;
    FG_TRY(pane_turn(plan, who, pane_id, &turn));
    if (plan->pre.active && plan->pre.input == input)
        return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: pane %lld of input %d was prefetched: feed it with flockgpu_plan_feed_pane(.., NULL, NULL, 0) first", who,
                    (long long)plan->pre.pane, plan->pre.input);
    // every check of the feed first: a refused feed must leave the ring as it was
    ColumnsCheck ck;
    ck.nothing = true;
    if (rows > 0 || n_cols > 0) FG_TRY(columns_check(plan, input, cols, n_cols, rows, who, ck));
    plan->col_stats.clear();
    FG_TRY(pane_begin(plan, &turn));
    if (ck.nothing) return FLOCKGPU_OK;   // an empty pane still advances the ring
    LeafData &ld = plan->leaves[(size_t)input];
    const LeafSnapshot before(ld);
    const int rc = columns_apply(plan, input, cols, rows, 0, ck);
    if (rc != FLOCKGPU_OK) {
        if (!plan->ring_q5) before.restore(ld);   // (columns_apply went back to these cursors itself; q5's state ring: the begun pane stays begun and empty)
        pane_undo(plan, turn);
        return rc;
    }
    pane_fed(plan, ld, before);
    return FLOCKGPU_OK;
}

int flockgpu_plan_result_columns(const flockgpu_plan *plan, flockgpu_text_column *out, int32_t capacity, int32_t *n_cols, int64_t *rows) {
    if (!plan) return FLOCKGPU_ERR_INVALID;
    flockgpu_ctx *ctx = plan->ctx;
    const Node *root = plan->ir.root.get();
    const int32_t n = (int32_t)root->schema.size();
    if (n_cols) *n_cols = n;
    if (rows) *rows = 0;
    if (!plan->has_retained) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_result_columns: the plan holds no retained result (flockgpu_plan_execute_retain)");
    if (!out || capacity < n) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_result_columns: room for %d columns, the result has %d", out ? capacity : 0, n);
    const Table &t = plan->retained;
    if ((int32_t)t.cols.size() != n) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_result_columns: the retained result has %d columns, the root's schema %d", (int)t.cols.size(), n);
    FG_HIP(ctx, hipSetDevice(ctx->device));
    // what an all_null column (MAX over no rows) and the columns of an empty result point at: zeros -- values, offsets and validity alike
    const size_t zero_bytes = (size_t)std::max<int64_t>(t.rows, 0) * 8 + 64;
    uint8_t *zeros = nullptr;
    bool zeros_ready = false;
    auto need_zeros = [&]() -> int {
        if (zeros_ready) return FLOCKGPU_OK;
        FG_TRY(arena_get_t(ctx, node_key(plan, root, "zeros").c_str(), zero_bytes, &zeros));
        FG_HIP(ctx, hipMemsetAsync(zeros, 0, zero_bytes, ctx->stream));
        zeros_ready = true;
        return FLOCKGPU_OK;
    };
    for (int32_t c = 0; c < n; ++c) {
        const Field &f = root->schema[(size_t)c];
        const DevColumn &col = t.cols[(size_t)c].c;
        flockgpu_text_column &o = out[c];
        o.name = f.name.c_str();
        o.type = text_type_of(f);
        o.values = nullptr;
        o.valid = nullptr;
        o.utf8 = flockgpu_utf8{nullptr, nullptr};
        const bool utf8 = f.type == ColType::UTF8;
        const bool absent = col.all_null || (utf8 ? !col.offsets || !col.values : !col.values);
        if (absent) {
            if (!col.all_null && t.rows > 0) return fail(ctx, FLOCKGPU_ERR_INVALID, "plan_result_columns: column '%s' of the retained result holds no data", f.name.c_str());
            FG_TRY(need_zeros());
            if (utf8) o.utf8 = flockgpu_utf8{reinterpret_cast<const int32_t *>(zeros), zeros};
            else o.values = zeros;
            if (col.all_null) o.valid = zeros;
            continue;
        }
        if (utf8) o.utf8 = flockgpu_utf8{col.offsets, static_cast<const uint8_t *>(col.values)};
        else o.values = col.values;
        o.valid = col.valid;
    }
    if (rows) *rows = t.rows;
    return FLOCKGPU_OK;
}
