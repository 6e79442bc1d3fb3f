// Event-time panes (panes.hpp, A-PN1..11): flockgpu_pane_split.
//   pane_census_kernel  the streaming pass: min t, max t, the first NULL row and whether the rows are in pane order, over 8 bytes a row (plus the
//                       validity bytes).  Tiles of kPaneTile rows; every lane asks for its sixteen 16-byte chunks of the tile (and its two chunks of
//                       the tile's validity bytes) before it looks at any of them.  A row can break pane order only where t[i] < t[i - 1]: only such
//                       a descent divides.  The row in front of a lane's pair comes from the lane below (one shuffle); lane 0 of a wave reads it
//                       itself -- for a tile's first row that is the previous tile's last.  Wave and workgroup reductions, one atomic per value and
//                       workgroup; the workgroup that takes the last ticket writes the answers to pinned memory and leaves the accumulators zero.
//   pane_bounds_kernel  rows in pane order: one lower-bound search per pane on the timestamp column itself, the results to pinned memory.
//   pane_ids_kernel     otherwise: pane ids relative to the first pane, for radix_sort_pairs / sorted_key_offsets (sort.hpp).
#include "panes.hpp"
#include "plan_source.hpp"
#include "sort.hpp"

namespace flockgpu {
namespace {

using namespace panes;

constexpr int kPaneIters = kPaneTile / (kBlock * 2);   // 16-byte chunks (two rows) per lane and tile
static_assert(kPaneIters * kBlock * 2 == kPaneTile, "a tile is a whole number of 16-byte chunks per lane");
static_assert(kPaneTile / 16 <= 2 * kBlock, "a tile's validity bytes are at most two 16-byte chunks per lane");

// the accumulators (all zero between calls): every one is raised with atomicMax / atomicOr, so zero is "nothing seen"
constexpr int kAccMinInv = 0;    // ~key(min t)
constexpr int kAccMax = 1;       // key(max t)
constexpr int kAccNullInv = 2;   // ~(first NULL row); 0: none
constexpr int kAccBad = 3;       // 1: a row lies in a pane below its predecessor's
constexpr int kAccTicket = 4;
constexpr int kAccWords = 5;
// the answers in pinned memory: 32-bit halves, so that no word can look like kPinnedPending
constexpr int kOutMinLo = 0, kOutMinHi = 1, kOutMaxLo = 2, kOutMaxHi = 3, kOutNull = 4, kOutBad = 5, kOutWords = 6;
constexpr uint64_t kNoNull = uint64_t(1) << 32;

__device__ __forceinline__ uint64_t order_key(int64_t t) { return (uint64_t)t ^ (uint64_t(1) << 63); }   // unsigned order = signed order
__device__ __forceinline__ int64_t from_key(uint64_t k) { return (int64_t)(k ^ (uint64_t(1) << 63)); }

// The index of the first zero byte of w (little-endian), or -1.
__device__ __forceinline__ int first_zero_byte(uint32_t w) {
    const uint32_t z = (w - 0x01010101u) & ~w & 0x80808080u;   // (the lowest set bit marks the lowest zero byte exactly: borrows only travel upwards)
    return z ? (__ffs((int)z) - 1) >> 3 : -1;
}
__device__ __forceinline__ int first_zero_byte16(const uint4 &q) {
    int i = first_zero_byte(q.x);
    if (i >= 0) return i;
    i = first_zero_byte(q.y);
    if (i >= 0) return 4 + i;
    i = first_zero_byte(q.z);
    if (i >= 0) return 8 + i;
    i = first_zero_byte(q.w);
    return i >= 0 ? 12 + i : -1;
}

__global__ __launch_bounds__(kBlock) void pane_census_kernel(const int64_t *__restrict__ t, const uint8_t *__restrict__ valid, int64_t rows, int64_t origin,
                                                             int64_t hop, unsigned long long *__restrict__ acc, uint64_t *__restrict__ h_out) {
    __shared__ int64_t s_min[kWavesPerBlock], s_max[kWavesPerBlock], s_null[kWavesPerBlock];
    __shared__ int s_bad[kWavesPerBlock];
    __shared__ int s_last;
    const int32_t tid = (int32_t)threadIdx.x;
    const int lane = lane_id();
    // the column from its first 16-byte aligned row on: `head` (0 or 1) rows in front of it
    const int64_t head = (reinterpret_cast<uintptr_t>(t) & 8u) ? 1 : 0;
    const int64_t *__restrict__ tb = t + head;
    const int64_t body = rows - head;   // (rows >= 1)
    const int32_t n_tiles = (int32_t)((rows + kPaneTile - 1) / kPaneTile);   // tiles of the validity bytes; the column's own are as many or one fewer
    int64_t mn = INT64_MAX, mx = INT64_MIN, first_null = INT64_MAX;
    bool bad = false;
    if (head && blockIdx.x == 0 && tid == 0) mn = mx = t[0];   // (row 0 has no predecessor)
    for (int32_t tile = (int32_t)blockIdx.x; tile < n_tiles; tile += (int32_t)gridDim.x) {
        const int64_t b0 = (int64_t)tile * kPaneTile;
        const int64_t left = body - b0;
        const int32_t n_here = (int32_t)(left < kPaneTile ? (left > 0 ? left : 0) : kPaneTile);
        // ---- every load of the tile is asked for before any is looked at
        uint4 q[kPaneIters];
        int64_t pv[kPaneIters];   // lane 0 of a wave: the row in front of its pair
#pragma unroll
        for (int it = 0; it < kPaneIters; ++it) {
            const int32_t e = (it * kBlock + tid) * 2;
            q[it] = make_uint4(0, 0, 0, 0);
            pv[it] = 0;
            if (e + 1 < n_here) {
                q[it] = stream_load4u(reinterpret_cast<const uint32_t *>(tb + b0 + e));
            } else if (e < n_here) {   // the column's last row, when the aligned part holds an odd number
                const int64_t v = tb[b0 + e];
                q[it].x = (uint32_t)(uint64_t)v;
                q[it].y = (uint32_t)((uint64_t)v >> 32);
            }
            if (lane == 0 && e < n_here && head + b0 + e > 0) pv[it] = t[head + b0 + e - 1];
        }
        uint4 v0 = make_uint4(~0u, ~0u, ~0u, ~0u), v1 = v0;
        uint32_t vh = 1, vt = 1;
        int32_t n_v = 0, v_head = 0, v_n16 = 0, v_tail0 = 0;
        if (valid) {   // (uniform) the tile's validity bytes: the aligned middle in 16-byte chunks, the ragged ends byte by byte
            const uint8_t *__restrict__ p = valid + b0;
            const int64_t v_left = rows - b0;
            n_v = (int32_t)(v_left < kPaneTile ? v_left : kPaneTile);
            const int32_t lead = (int32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u);
            v_head = lead < n_v ? lead : n_v;
            v_n16 = (n_v - v_head) >> 4;
            v_tail0 = v_head + (v_n16 << 4);
            if (tid < v_n16) v0 = stream_load4u(reinterpret_cast<const uint32_t *>(p + v_head + 16 * tid));
            if (tid + kBlock < v_n16) v1 = stream_load4u(reinterpret_cast<const uint32_t *>(p + v_head + 16 * (tid + kBlock)));
            if (tid < v_head) vh = p[tid];
            if (tid < n_v - v_tail0) vt = p[v_tail0 + tid];
        }
        // ---- the timestamps
#pragma unroll
        for (int it = 0; it < kPaneIters; ++it) {
            const int32_t e = (it * kBlock + tid) * 2;
            const int64_t a = (int64_t)((uint64_t)q[it].x | ((uint64_t)q[it].y << 32));
            const int64_t b = (int64_t)((uint64_t)q[it].z | ((uint64_t)q[it].w << 32));
            int64_t prev = __shfl_up((long long)b, 1, 64);   // (a lane that holds a row has a lane below with a whole pair)
            if (lane == 0) prev = pv[it];
            const bool has_a = e < n_here, has_b = e + 1 < n_here, has_prev = head + b0 + e > 0;
            if (has_a) {
                mn = a < mn ? a : mn;
                mx = a > mx ? a : mx;
                if (has_prev && a < prev && !bad) bad = wide_less(pane_wide(a, origin, hop), pane_wide(prev, origin, hop));
            }
            if (has_b) {
                mn = b < mn ? b : mn;
                mx = b > mx ? b : mx;
                if (b < a && !bad) bad = wide_less(pane_wide(b, origin, hop), pane_wide(a, origin, hop));
            }
        }
        // ---- the validity bytes: this lane's first NULL row of the tile (its chunks ascend: head bytes, chunk tid, chunk tid + kBlock, tail bytes)
        if (valid) {
            int64_t at = INT64_MAX;
            if (tid < n_v - v_tail0 && vt == 0) at = b0 + v_tail0 + tid;
            int z = tid + kBlock < v_n16 ? first_zero_byte16(v1) : -1;
            if (z >= 0) at = b0 + v_head + 16 * (tid + kBlock) + z;
            z = tid < v_n16 ? first_zero_byte16(v0) : -1;
            if (z >= 0) at = b0 + v_head + 16 * tid + z;
            if (tid < v_head && vh == 0) at = b0 + tid;
            first_null = at < first_null ? at : first_null;
        }
    }
    // ---- wave, then workgroup, then one atomic per value
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t omn = __shfl_xor((long long)mn, o, 64), omx = __shfl_xor((long long)mx, o, 64), onl = __shfl_xor((long long)first_null, o, 64);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
        first_null = onl < first_null ? onl : first_null;
    }
    const int any_bad = __any((int)bad);
    if (lane == 0) {
        s_min[tid >> 6] = mn;
        s_max[tid >> 6] = mx;
        s_null[tid >> 6] = first_null;
        s_bad[tid >> 6] = any_bad;
    }
    __syncthreads();
    if (tid == 0) {
        int all_bad = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) {
            mn = s_min[w] < mn ? s_min[w] : mn;
            mx = s_max[w] > mx ? s_max[w] : mx;
            first_null = s_null[w] < first_null ? s_null[w] : first_null;
            all_bad |= s_bad[w];
        }
        // (a workgroup that saw no row adds ~key(INT64_MAX) = 0 and key(INT64_MIN) = 0: nothing)
        if (mn != INT64_MAX) atomicMax(&acc[kAccMinInv], (unsigned long long)~order_key(mn));
        if (mx != INT64_MIN) atomicMax(&acc[kAccMax], (unsigned long long)order_key(mx));
        if (first_null != INT64_MAX) atomicMax(&acc[kAccNullInv], (unsigned long long)~(uint64_t)first_null);
        if (all_bad) atomicOr(&acc[kAccBad], 1ull);
        __threadfence();
        s_last = atomicAdd(&acc[kAccTicket], 1ull) == (unsigned long long)gridDim.x - 1ull;
    }
    __syncthreads();
    if (!s_last || tid != 0) return;
    __threadfence();
    const int64_t t_min = from_key(~(uint64_t)atomicExch(&acc[kAccMinInv], 0ull));
    const int64_t t_max = from_key((uint64_t)atomicExch(&acc[kAccMax], 0ull));
    const uint64_t null_inv = (uint64_t)atomicExch(&acc[kAccNullInv], 0ull);
    const uint64_t was_bad = (uint64_t)atomicExch(&acc[kAccBad], 0ull);
    atomicExch(&acc[kAccTicket], 0ull);
    h_out[kOutMinLo] = (uint64_t)(uint32_t)(uint64_t)t_min;
    h_out[kOutMinHi] = (uint64_t)t_min >> 32;
    h_out[kOutMaxLo] = (uint64_t)(uint32_t)(uint64_t)t_max;
    h_out[kOutMaxHi] = (uint64_t)t_max >> 32;
    h_out[kOutNull] = null_inv ? ~null_inv : kNoNull;
    h_out[kOutBad] = was_bad;
}

// bounds[k], 0 < k < n_panes: the first row whose t is not below threshold(first_pane + k) (A-PN8: the threshold fits Int64 and wraps nowhere).
__global__ __launch_bounds__(kBlock) void pane_bounds_kernel(const int64_t *__restrict__ t, int64_t rows, int64_t origin, int64_t hop, int64_t first_pane,
                                                             int32_t n_panes, uint64_t *__restrict__ h_bounds) {
    const int32_t k = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (k > n_panes) return;
    int64_t lo = 0, hi = rows;
    if (k == 0) hi = 0;
    else if (k == n_panes) lo = rows;
    else {
        const int64_t thr = (int64_t)((uint64_t)origin + (uint64_t)(first_pane + k) * (uint64_t)hop);
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (t[mid] >= thr) hi = mid;
            else lo = mid + 1;
        }
    }
    h_bounds[k] = (uint64_t)lo;
}

__global__ __launch_bounds__(kBlock) void pane_ids_kernel(const int64_t *__restrict__ t, int64_t rows, int64_t origin, int64_t hop, int64_t first_pane,
                                                          int32_t *__restrict__ ids) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < rows; i += stride) {
        int64_t p = first_pane;
        (void)pane_of(t[i], origin, hop, &p);   // (fits: the panes of min t and max t do)
        ids[i] = (int32_t)(p - first_pane);
    }
}

// The accumulators are zero between calls (the kernel leaves them so); a buffer seen for the first time is cleared once.
int census_acc(flockgpu_ctx *ctx, unsigned long long **acc) {
    FG_TRY(arena_get_t(ctx, "pane_split.acc", (size_t)kAccWords, acc));
    std::vector<int64_t> &seen = ctx->host_i64["pane_split.acc"];
    if (seen.size() != 1 || seen[0] != (int64_t)reinterpret_cast<uintptr_t>(*acc)) {
        FG_TRY(fill_words(ctx, FillList().add(*acc, 0u, (uint64_t)kAccWords * 2)));
        seen.assign(1, (int64_t)reinterpret_cast<uintptr_t>(*acc));
    }
    return FLOCKGPU_OK;
}

}  // namespace

int pane_split(flockgpu_ctx *ctx, const int64_t *time_ms, const uint8_t *valid, int64_t rows, int64_t origin_ms, int64_t hop_ms, int32_t capacity,
               int64_t *bounds, PaneSplit *out) {
    *out = PaneSplit{};
    if (rows == 0) {
        bounds[0] = 0;
        return FLOCKGPU_OK;
    }
    // ---- the streaming pass: one launch, one wait
    unsigned long long *acc = nullptr;
    uint64_t *h = nullptr;
    FG_TRY(census_acc(ctx, &acc));
    FG_TRY(pinned_get_t(ctx, "pane_split.census", (size_t)kOutWords, &h));
    pinned_pending(h, kOutWords);
    {
        LaunchScope ls(ctx, "pane_census_kernel");
        const unsigned grid = (unsigned)std::min<int64_t>(div_up(rows, (int64_t)kPaneTile), (int64_t)ctx->num_cus * kStreamBlocksPerCu);
        hipLaunchKernelGGL(pane_census_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, time_ms, valid, rows, origin_ms, hop_ms, acc, h);
    }
    FG_TRY(check_launch(ctx, "pane_census_kernel"));
    FG_TRY(wait_pinned(ctx, h, kOutWords));
    const int64_t t_min = (int64_t)(h[kOutMinLo] | (h[kOutMinHi] << 32)), t_max = (int64_t)(h[kOutMaxLo] | (h[kOutMaxHi] << 32));
    if (valid && h[kOutNull] != kNoNull)
        return fail(ctx, FLOCKGPU_ERR_INVALID, "pane_split: row %lld holds a NULL timestamp: a row without a time lies in no pane", (long long)h[kOutNull]);
    int64_t first = 0, last = 0;
    const bool first_fits = panes::pane_of(t_min, origin_ms, hop_ms, &first);
    if (!first_fits || !panes::pane_of(t_max, origin_ms, hop_ms, &last))
        return fail(ctx, FLOCKGPU_ERR_INVALID, "pane_split: the pane of timestamp %lld (origin %lld, hop %lld) does not fit Int64",
                    (long long)(first_fits ? t_max : t_min), (long long)origin_ms, (long long)hop_ms);
    const uint64_t span = (uint64_t)last - (uint64_t)first;   // (last >= first: pane() is monotone)
    if (span >= (uint64_t)capacity)
        return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "pane_split: the rows span panes %lld to %lld, more than the capacity of %d panes", (long long)first,
                    (long long)last, capacity);
    const int32_t n = (int32_t)span + 1;
    out->first_pane = first;
    out->n_panes = n;
    if (!h[kOutBad]) {   // ---- rows in pane order: the bounds by search, one small launch, one wait
        if (n > 1) {
            uint64_t *hb = nullptr;
            FG_TRY(pinned_get_t(ctx, "pane_split.bounds", (size_t)n + 1, &hb));
            pinned_pending(hb, n + 1);
            {
                LaunchScope ls(ctx, "pane_bounds_kernel");
                hipLaunchKernelGGL(pane_bounds_kernel, dim3((unsigned)div_up((int64_t)n + 1, kBlock)), dim3(kBlock), 0, ctx->stream, time_ms, rows, origin_ms, hop_ms,
                                   first, n, hb);
            }
            FG_TRY(check_launch(ctx, "pane_bounds_kernel"));
            FG_TRY(wait_pinned(ctx, hb, n + 1));
            for (int32_t k = 0; k <= n; ++k) bounds[k] = (int64_t)hb[k];
        } else {
            bounds[0] = 0;
            bounds[1] = rows;
        }
        return FLOCKGPU_OK;
    }
    // ---- otherwise: pane ids relative to the first pane, a stable sort over the bits they need, the panes' first positions
    int32_t *ids = nullptr, *sorted = nullptr;
    uint32_t *list = nullptr;
    int64_t *d_off = nullptr, *h_off = nullptr;
    FG_TRY(arena_get_t(ctx, "pane_split.ids", (size_t)rows + 4, &ids));
    FG_TRY(arena_get_t(ctx, "pane_split.off", (size_t)n + 1, &d_off));
    FG_TRY(pinned_get_t(ctx, "pane_split.off", (size_t)n + 1, &h_off));
    {
        LaunchScope ls(ctx, "pane_ids_kernel");
        const unsigned grid = (unsigned)std::min<int64_t>(div_up(rows, kBlock), (int64_t)ctx->num_cus * 8);
        hipLaunchKernelGGL(pane_ids_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, time_ms, rows, origin_ms, hop_ms, first, ids);
    }
    FG_TRY(check_launch(ctx, "pane_ids_kernel"));
    int bits = 1;
    while (bits < 17 && ((uint32_t)(n - 1) >> bits)) ++bits;
    FG_TRY(radix_sort_pairs(ctx, "pane_split.sort", ids, nullptr, rows, 0, bits, &sorted, &list));
    FG_TRY(sorted_key_offsets(ctx, sorted, rows, n, d_off));
    FG_HIP(ctx, hipMemcpyAsync(h_off, d_off, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream));
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int32_t k = 0; k <= n; ++k) bounds[k] = h_off[k];
    out->row_list = reinterpret_cast<const int32_t *>(list);
    return FLOCKGPU_OK;
}

}  // namespace flockgpu

extern "C" {

int flockgpu_pane_split(flockgpu_ctx *ctx, const int64_t *time_ms, const uint8_t *valid, int64_t rows, int64_t origin_ms, int64_t hop_ms, int32_t capacity,
                        int64_t *first_pane, int32_t *n_panes, int64_t *bounds, const int32_t **row_list) {
    using namespace flockgpu;
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    if (!first_pane || !n_panes || !bounds || !row_list || (rows > 0 && !time_ms)) return fail(ctx, FLOCKGPU_ERR_INVALID, "pane_split: null argument");
    if (hop_ms <= 0) return fail(ctx, FLOCKGPU_ERR_INVALID, "pane_split: a hop of %lld ms", (long long)hop_ms);
    if (capacity < 1 || capacity > panes::kPaneMaxCapacity)
        return fail(ctx, FLOCKGPU_ERR_INVALID, "pane_split: a capacity of %d panes (1 to %d)", capacity, panes::kPaneMaxCapacity);
    if (rows < 0 || rows >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_INVALID, "pane_split: %lld rows (0 to 2^31 - 1)", (long long)rows);
    if (reinterpret_cast<uintptr_t>(time_ms) & 7u) return fail(ctx, FLOCKGPU_ERR_INVALID, "pane_split: the timestamp column is not aligned to its element size");
    FG_HIP(ctx, hipSetDevice(ctx->device));
    PaneSplit ps;
    FG_TRY(pane_split(ctx, time_ms, valid, rows, origin_ms, hop_ms, capacity, bounds, &ps));
    *first_pane = ps.first_pane;
    *n_panes = ps.n_panes;
    *row_list = ps.row_list;
    return FLOCKGPU_OK;
}

int flockgpu_take_u8(flockgpu_ctx *ctx, const uint8_t *src, const int32_t *rows, int64_t n, uint8_t *out) {
    using namespace flockgpu;
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    if (n < 0 || (n > 0 && (!src || !rows || !out))) return fail(ctx, FLOCKGPU_ERR_INVALID, "take_u8: null argument");
    FG_HIP(ctx, hipSetDevice(ctx->device));
    TailTakeCols tk;
    tk.src[0] = src;
    tk.out[0] = out;
    tk.width[0] = 1;
    tk.n = 1;
    return take_to_tail(ctx, tk, rows, n);
}

}  // extern "C"
