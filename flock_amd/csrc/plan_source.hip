// Device-side ingest of a plan leaf (plan_source.hpp): the census of the fed validity bytes, the rebased append of Utf8 offsets and the take
// that writes a row list's rows at a misaligned tail.  Streaming kernels for gfx950 (wave64), shaped like the library's others: 16-byte loads and
// stores wherever both ends allow them, the ragged ends element by element, no workgroup waiting for another.
#include "plan_source.hpp"

namespace flockgpu {
namespace {

constexpr int kAccKept = kCensusCols;         // the accumulators: NULLs per column, rows kept, the ticket of the workgroups that are done
constexpr int kAccTicket = kCensusCols + 1;
constexpr int kAccWords = kCensusCols + 2;
constexpr int kStagePad = 32;

// ---- census.  Tiles of kFlagTile rows.  A column's 8192 validity bytes of the tile are staged in LDS with 16-byte loads: byte i of the
// tile sits at s_stage[mis + i], mis = the source address modulo 16, so every aligned 16-byte chunk of the source is an aligned chunk of the
// stage; the bytes in front of the first whole chunk and behind the last are copied one by one (nothing outside [p, p + n_here) is read).  Every
// lane then reads its 4 x 8 rows of the flag-tile layout (scan.hpp) as eight dwords, realigned from two aligned LDS words.  The workgroup that
// takes the last ticket hands the totals (and the Utf8 columns' end offsets) to the host and leaves the accumulators zero for the next call.
__global__ __launch_bounds__(kBlock) void feed_census_kernel(CensusArgs a, int64_t rows, uint32_t *__restrict__ flag_words, uint32_t *__restrict__ counts,
                                                             unsigned long long *__restrict__ acc, uint64_t *__restrict__ h_out) {
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[kFlagTile + kStagePad];
    __shared__ uint32_t s_count[kCensusCols + 1];   // this workgroup's NULLs per column and rows kept (below 2^31: the relation's rows are)
    __shared__ int s_last;
    const int32_t tid = (int32_t)threadIdx.x;
    if (tid <= kCensusCols) s_count[tid] = 0;
    __syncthreads();
    const int32_t rel0 = flag_rel0();
    const int32_t n_tiles = a.n_valid > 0 ? (int32_t)((rows + kFlagTile - 1) / kFlagTile) : 0;   // (Utf8 columns alone: nothing to walk, only their end offsets to fetch)
    // a workgroup walks tiles b, b + G, ...: its counts gather in LDS and reach the global accumulators ONCE per column, not once per tile (adds of
    // many workgroups on one address queue up behind each other)
    for (int32_t tile = (int32_t)blockIdx.x; tile < n_tiles; tile += (int32_t)gridDim.x) {
        const int64_t tile_begin = (int64_t)tile * kFlagTile;
        const int64_t left = rows - tile_begin;
        const int32_t n_here = (int32_t)(left < kFlagTile ? left : kFlagTile);
        uint32_t inb = 0;   // this lane's rows that exist
#pragma unroll
        for (int it = 0; it < kFlagIters; ++it)
#pragma unroll
            for (int j = 0; j < 4; ++j) inb |= (uint32_t)(rel0 + it * 256 + j < n_here) << (it * 4 + j);
        uint32_t flags = inb;
        for (int c = 0; c < a.n_valid; ++c) {   // (uniform trip count)
            const uint8_t *__restrict__ p = a.valid[c] + tile_begin;
            const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
            const int32_t lead = (int32_t)((16u - mis) & 15u);
            const int32_t head = lead < n_here ? lead : n_here;
            const int32_t n16 = (n_here - head) >> 4;   // <= 512: at most two chunks per thread, both asked for before either is stored
            const int32_t tail0 = head + (n16 << 4);
            uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
            if (tid < n16) q0 = stream_load4u(reinterpret_cast<const uint32_t *>(p + head + 16 * tid));
            if (tid + kBlock < n16) q1 = stream_load4u(reinterpret_cast<const uint32_t *>(p + head + 16 * (tid + kBlock)));
            if (tid < head) s_stage[mis + (uint32_t)tid] = p[tid];
            if (tid < n_here - tail0) s_stage[mis + (uint32_t)(tail0 + tid)] = p[tail0 + tid];
            if (tid < n16) *reinterpret_cast<uint4 *>(s_stage + mis + head + 16 * tid) = q0;
            if (tid + kBlock < n16) *reinterpret_cast<uint4 *>(s_stage + mis + head + 16 * (tid + kBlock)) = q1;
            __syncthreads();
            const uint32_t *s_words = reinterpret_cast<const uint32_t *>(s_stage);
            const uint32_t sh = (mis & 3u) * 8u;
            uint32_t nullbits = 0;
#pragma unroll
            for (int it = 0; it < kFlagIters; ++it) {
                const uint32_t at = (mis + (uint32_t)(rel0 + it * 256)) >> 2;   // (rel0 is a multiple of 4: the byte inside the word is mis & 3 for every lane)
                const uint32_t w0 = s_words[at], w1 = s_words[at + 1];
                const uint32_t v = sh ? (w0 >> sh) | (w1 << (32u - sh)) : w0;
#pragma unroll
                for (int j = 0; j < 4; ++j) nullbits |= (uint32_t)(((v >> (8 * j)) & 0xffu) == 0u) << (it * 4 + j);
            }
            nullbits &= inb;   // (stage bytes past the tile's rows are whatever the last column left there)
            __syncthreads();   // (the next column overwrites the stage)
            if ((a.droppable >> c) & 1ull) flags &= ~nullbits;
            const uint32_t incl = wave_incl_scan_u32((uint32_t)__popc(nullbits));
            if (lane_id() == 63 && incl) atomicAdd(&s_count[c], incl);
        }
        if (flag_words) {
            store_flags_and_counts(flags, tile, flag_words, counts);
            const uint32_t incl = wave_incl_scan_u32((uint32_t)__popc(flags));
            if (lane_id() == 63 && incl) atomicAdd(&s_count[kAccKept], incl);
        }
    }
    __syncthreads();
    if (tid <= kCensusCols && s_count[tid]) atomicAdd(&acc[tid], (unsigned long long)s_count[tid]);
    __threadfence();
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(&acc[kAccTicket], 1ull) == (unsigned long long)gridDim.x - 1ull;
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    if (tid < kCensusCols) h_out[tid] = tid < a.n_valid ? (uint64_t)atomicExch(&acc[tid], 0ull) : 0ull;
    if (tid == kAccKept) {
        const uint64_t kept = (uint64_t)atomicExch(&acc[kAccKept], 0ull);
        h_out[kAccKept] = flag_words ? kept : (uint64_t)rows;
    }
    if (tid < a.n_utf8) {
        h_out[kCensusCols + 1 + 2 * tid] = (uint64_t)(uint32_t)a.offsets[tid][0];
        h_out[kCensusCols + 2 + 2 * tid] = (uint64_t)(uint32_t)a.offsets[tid][rows];
    }
    if (tid == 0) atomicExch(&acc[kAccTicket], 0ull);
}

// ---- rebased append of Utf8 offsets: the 16-byte aligned middle of the DESTINATION with 16-byte stores, its ragged ends word by word; the source
// is read with 16-byte loads where it happens to be aligned with the destination, word by word (neighbouring lanes, neighbouring words) otherwise.
__global__ __launch_bounds__(kBlock) void offsets_rebase_kernel(int32_t *__restrict__ dst, const int32_t *__restrict__ src, int64_t n, int32_t cursor) {
    const uint32_t base = (uint32_t)cursor - (uint32_t)src[0];
    const int32_t *__restrict__ s = src + 1;
    const int64_t lead = (int64_t)((4u - (uint32_t)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3u)) & 3u);
    const int64_t head = lead < n ? lead : n;
    const int64_t n4 = (n - head) >> 2;
    const int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
    if (t0 < head) dst[t0] = (int32_t)((uint32_t)s[t0] + base);
    const bool src_aligned = (reinterpret_cast<uintptr_t>(s + head) & 15u) == 0;   // (uniform)
    for (int64_t q = t0; q < n4; q += stride) {
        const int64_t e = head + 4 * q;
        uint4 v;
        if (src_aligned) {
            v = stream_load4u(reinterpret_cast<const uint32_t *>(s + e));
        } else {
            v = make_uint4((uint32_t)s[e], (uint32_t)s[e + 1], (uint32_t)s[e + 2], (uint32_t)s[e + 3]);
        }
        stream_store4(dst + e, make_uint4(v.x + base, v.y + base, v.z + base, v.w + base));
    }
    const int64_t tail0 = head + 4 * n4;
    if (t0 < n - tail0) dst[tail0 + t0] = (int32_t)((uint32_t)s[tail0 + t0] + base);
}

// ---- tail take: gather_multi_kernel's shape (the row list read once, four rows per lane in one 16-byte load, every column's four values in flight
// together) with validity bytes as a third width and a destination that may be misaligned: 16-byte (validity: 4-byte) stores where out[c] allows
// them, element by element otherwise.  The n & 3 rows behind the last whole group of four go one per thread.
template <typename T>
__device__ __forceinline__ void tail_take4(const void *src, void *out, const int4 &r, int64_t e) {
    const T *__restrict__ s = static_cast<const T *>(src);
    T *__restrict__ o = static_cast<T *>(out) + e;
    const T v0 = s[r.x], v1 = s[r.y], v2 = s[r.z], v3 = s[r.w];
    o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3;
}
__global__ __launch_bounds__(kBlock) void take_tail_kernel(TailTakeCols cols, const int32_t *__restrict__ rows, int64_t n) {
    const int64_t n4 = n >> 2;
    const int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t q = t0; q < n4; q += stride) {
        const int4 r = *reinterpret_cast<const int4 *>(rows + q * 4);   // (the list is an arena buffer: 16-byte aligned)
        const int64_t e = q * 4;
        for (int c = 0; c < cols.n; ++c) {   // (uniform trip count and branches)
            const bool vec = (reinterpret_cast<uintptr_t>(cols.out[c]) & 15u) == 0;
            if (cols.width[c] == 4) {
                if (vec) {
                    const uint32_t *__restrict__ s = static_cast<const uint32_t *>(cols.src[c]);
                    stream_store4(static_cast<uint32_t *>(cols.out[c]) + e, make_uint4(s[r.x], s[r.y], s[r.z], s[r.w]));
                } else {
                    tail_take4<uint32_t>(cols.src[c], cols.out[c], r, e);
                }
            } else if (cols.width[c] == 8) {
                if (vec) {
                    const uint64_t *__restrict__ s = static_cast<const uint64_t *>(cols.src[c]);
                    const uint64_t v0 = s[r.x], v1 = s[r.y], v2 = s[r.z], v3 = s[r.w];
                    uint64_t *o = static_cast<uint64_t *>(cols.out[c]) + e;
                    stream_store4(o, make_uint4((uint32_t)v0, (uint32_t)(v0 >> 32), (uint32_t)v1, (uint32_t)(v1 >> 32)));
                    stream_store4(o + 2, make_uint4((uint32_t)v2, (uint32_t)(v2 >> 32), (uint32_t)v3, (uint32_t)(v3 >> 32)));
                } else {
                    tail_take4<uint64_t>(cols.src[c], cols.out[c], r, e);
                }
            } else {
                const uint8_t *__restrict__ s = static_cast<const uint8_t *>(cols.src[c]);
                if ((reinterpret_cast<uintptr_t>(cols.out[c]) & 3u) == 0) {
                    const uint32_t v = (uint32_t)s[r.x] | ((uint32_t)s[r.y] << 8) | ((uint32_t)s[r.z] << 16) | ((uint32_t)s[r.w] << 24);
                    *reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(cols.out[c]) + e) = v;
                } else {
                    tail_take4<uint8_t>(cols.src[c], cols.out[c], r, e);
                }
            }
        }
    }
    const int64_t e = n4 * 4 + t0;
    if (t0 < (n & 3)) {
        const int32_t r = rows[e];
        for (int c = 0; c < cols.n; ++c) {
            if (cols.width[c] == 4) static_cast<uint32_t *>(cols.out[c])[e] = static_cast<const uint32_t *>(cols.src[c])[r];
            else if (cols.width[c] == 8) static_cast<uint64_t *>(cols.out[c])[e] = static_cast<const uint64_t *>(cols.src[c])[r];
            else static_cast<uint8_t *>(cols.out[c])[e] = static_cast<const uint8_t *>(cols.src[c])[r];
        }
    }
}

}  // namespace

int feed_census_begin(flockgpu_ctx *ctx, const char *name, const CensusArgs &a, int64_t rows, CensusResult *out) {
    *out = CensusResult{};
    if (a.n_valid == 0 && a.n_utf8 == 0) return FLOCKGPU_OK;
    if (rows <= 0 || rows >= (int64_t(1) << 31) || a.n_valid < 0 || a.n_valid > kCensusCols || a.n_utf8 < 0 || a.n_utf8 > kCensusUtf8)
        return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: census of %lld rows, %d validity and %d Utf8 columns", name, (long long)rows, a.n_valid, a.n_utf8);
    const std::string base = name;
    const int32_t tiles = (int32_t)div_up(rows, (int64_t)kFlagTile);
    unsigned long long *acc = nullptr;
    uint64_t *h = nullptr;
    // (one set of accumulators per context, under a name no plan's destroy frees: the calls of a context follow each other on its stream)
    FG_TRY(arena_get_t(ctx, "plan_source.acc", (size_t)kAccWords, &acc));
    // the accumulators are zero between calls (the kernel leaves them so); a buffer seen for the first time is cleared once
    std::vector<int64_t> &seen = ctx->host_i64["plan_source.acc"];
    if (seen.size() != 1 || seen[0] != (int64_t)reinterpret_cast<uintptr_t>(acc)) {
        FG_TRY(fill_words(ctx, FillList().add(acc, 0u, (uint64_t)kAccWords * 2)));
        seen.assign(1, (int64_t)reinterpret_cast<uintptr_t>(acc));
    }
    if (a.droppable) {
        FG_TRY(arena_get_t(ctx, (base + ".flags").c_str(), (size_t)tiles * kBlock + 4, &out->flag_words));
        FG_TRY(arena_get_t(ctx, (base + ".counts").c_str(), (size_t)tiles * kWavesPerBlock + 4, &out->counts));
    }
    out->n_tiles = tiles;
    out->n_words = kCensusCols + 1 + 2 * a.n_utf8;
    FG_TRY(pinned_get_t(ctx, (base + ".census").c_str(), (size_t)kCensusCols + 1 + 2 * kCensusUtf8, &h));
    pinned_pending(h, out->n_words);
    out->h = h;
    {
        LaunchScope ls(ctx, "feed_census_kernel");
        const unsigned blocks = a.n_valid > 0 ? (unsigned)std::min<int64_t>(tiles, (int64_t)ctx->num_cus * 8) : 1u;   // (no validity: ONE workgroup fetches the Utf8 end offsets)
        hipLaunchKernelGGL(feed_census_kernel, dim3(blocks), dim3(kBlock), 0, ctx->stream, a, rows, out->flag_words, out->counts, acc, h);
    }
    return check_launch(ctx, "feed_census_kernel");
}

int feed_census_wait(flockgpu_ctx *ctx, const CensusResult &r) {
    if (!r.h) return FLOCKGPU_OK;   // (nothing was queued)
    return wait_pinned(ctx, r.h, r.n_words);
}

int feed_census_rows(flockgpu_ctx *ctx, const char *name, const CensusResult &r, int64_t rows, int64_t kept, const int32_t **out_rows) {
    const std::string base = name;
    int32_t *o_rows = nullptr;
    FG_TRY(arena_get_t(ctx, (base + ".rows").c_str(), (size_t)std::max<int64_t>(kept, 0) + 4, &o_rows));
    *out_rows = o_rows;
    if (kept <= 0) return FLOCKGPU_OK;
    if (!r.flag_words) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: the census kept no flags", name);
    int64_t sb = 0, se = rows;
    SegTiles st;
    FG_TRY(build_seg_tiles(ctx, (base + ".tiles").c_str(), &sb, &se, 1, kFlagTile, &st));   // (one segment from row 0: tile t = rows [8192 t, 8192 (t + 1)), as the census walks them)
    if (st.n_tiles != r.n_tiles) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: %d tiles for a census of %d", name, st.n_tiles, r.n_tiles);
    if (st.n_tiles <= 2048) {   // (no scan launch: gather.hpp, emit_flagged_rows_self; its total is the census' `kept`, nobody waits for it)
        int64_t *h_off = nullptr;
        FG_TRY(pinned_get_t(ctx, (base + ".off").c_str(), 2, &h_off));
        return emit_flagged_rows_self(ctx, st, r.flag_words, r.counts, o_rows, h_off);
    }
    uint64_t *tile_base = nullptr;
    FG_TRY(arena_get_t(ctx, (base + ".base").c_str(), (size_t)st.n_tiles + 1, &tile_base));
    FG_TRY(launch_tile_scan(ctx, r.counts, st.n_tiles, tile_base, nullptr, 0, nullptr));
    return emit_flagged_rows(ctx, st, r.flag_words, r.counts, tile_base, o_rows);
}

int append_offsets_rebased(flockgpu_ctx *ctx, int32_t *dst, const int32_t *src, int64_t n, int32_t cursor) {
    if (n <= 0) return FLOCKGPU_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>(div_up(div_up(n, 4) + 3, kBlock), (int64_t)ctx->num_cus * 8);
    {
        LaunchScope ls(ctx, "offsets_rebase_kernel");
        hipLaunchKernelGGL(offsets_rebase_kernel, dim3(blocks), dim3(kBlock), 0, ctx->stream, dst, src, n, cursor);
    }
    return check_launch(ctx, "offsets_rebase_kernel");
}

int take_to_tail(flockgpu_ctx *ctx, const TailTakeCols &cols, const int32_t *rows, int64_t n) {
    if (n <= 0 || cols.n <= 0) return FLOCKGPU_OK;
    if (cols.n > kGatherMulti) return fail(ctx, FLOCKGPU_ERR_INVALID, "take_to_tail: more than %d columns", kGatherMulti);
    if (reinterpret_cast<uintptr_t>(rows) & 15) return fail(ctx, FLOCKGPU_ERR_INVALID, "take_to_tail: the row list is not 16-byte aligned");
    const unsigned blocks = (unsigned)std::min<int64_t>(div_up(div_up(n, 4) + 3, kBlock), (int64_t)ctx->num_cus * 8);
    {
        LaunchScope ls(ctx, "take_tail_kernel");
        hipLaunchKernelGGL(take_tail_kernel, dim3(blocks), dim3(kBlock), 0, ctx->stream, cols, rows, n);
    }
    return check_launch(ctx, "take_tail_kernel");
}

}  // namespace flockgpu
