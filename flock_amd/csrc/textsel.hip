// Utf8-valued expressions (textsel.hpp): (selector, source table) -> an ordinary Utf8 column.
//   textsel_len_kernel    per row the chosen source's length -> a byte count per wave (the tile scan's input) and the validity bytes.
//   textsel_emit_kernel   offsets and bytes.  A lane owns FOUR CONSECUTIVE rows: the selector arrives as one 16-byte load, the validity as one
//                         4-byte load, and the lane's four offsets leave as ONE aligned 16-byte store (out_off[i] = where row i STARTS; the last
//                         tile adds out_off[rows]).  The tile's bytes are one contiguous range of the output: a tile of up to
//                         kTextStageBytes is assembled in LDS -- every value is read from its source as aligned dwords and written as aligned
//                         dwords (its first and last up to three bytes byte by byte) -- and streamed out as aligned 16-byte
//                         non-temporal stores; only the first and last 16-byte chunk of a tile, which it shares with its neighbours, go out
//                         byte by byte.  The source table lives in LDS (literals: the pool, read as aligned dwords -- every literal starts on a
//                         4-byte boundary).  Two instances of each kernel: kCols = false (literals alone: NEXMark q14's labels) has no global
//                         load besides the selector; a third, kSlices, reads a value's range through a slice source's per-row (begin, end) arrays
//                         (textslice.hpp) where the source has them -- the two instances without it are what they were.
//   textsel_emit_long_kernel  the bytes of every tile beyond the stage (long column values): the take's chunk-wise copy for long values, shared
//                         (utf8_chunks.hpp), over the tile's (address, length) list in LDS.
//   textsel_fill_kernel   a bare literal: offsets i * len and the literal over and over, 16 bytes per lane and step.
// Every row index is checked against `rows`; a selector value outside 0 .. k - 1 (the slot of a NULL holds anything) reads source 0 and, being
// NULL, contributes no byte.
#include <algorithm>

#include "gather.hpp"
#include "scan.hpp"
#include "textsel.hpp"
#include "utf8_chunks.hpp"

using namespace flockgpu;

namespace {

constexpr int kRowsPerLane = kTextTile / kBlock;   // 4
static_assert(kRowsPerLane == 4, "a lane's rows are one 16-byte selector load and one 16-byte offsets store");
static_assert(kTextStageBytes % 16 == 0, "rounds end on 16-byte chunks");
constexpr int kPoolWords = (int)(sizeof(TextSources::pool) / 4);

// the source table in LDS
struct SharedTable {
    const int32_t *offsets[kTextMaxSources];
    const uint8_t *bytes[kTextMaxSources];
    const uint8_t *valid[kTextMaxSources];
    uint32_t lit_off[kTextMaxSources], lit_len[kTextMaxSources];
    uint32_t pool[kPoolWords];
};

// ... with the slice sources' per-row arrays (kSlices)
struct SharedSliceTable : SharedTable {
    const int32_t *begin[kTextMaxSources];
    const int32_t *end[kTextMaxSources];
};
template <bool kSlices>
struct TableOf { using type = SharedTable; };
template <>
struct TableOf<true> { using type = SharedSliceTable; };

template <bool kCols, bool kSlices>
__device__ __forceinline__ void load_table(const TextSources &S, typename TableOf<kSlices>::type &t) {
    if (threadIdx.x < (unsigned)kTextMaxSources) {
        const TextSource &s = S.src[threadIdx.x];
        if (kCols) {
            t.offsets[threadIdx.x] = s.offsets;
            t.bytes[threadIdx.x] = s.bytes;
            t.valid[threadIdx.x] = s.valid;
        }
        if constexpr (kSlices) {
            t.begin[threadIdx.x] = s.begin;
            t.end[threadIdx.x] = s.end;
        }
        t.lit_off[threadIdx.x] = s.lit_off;
        t.lit_len[threadIdx.x] = s.lit_len;
    }
    for (int i = (int)threadIdx.x; i < kPoolWords; i += kBlock) t.pool[i] = S.pool[i];
    __syncthreads();
}

// offsets[r] and offsets[r + 1] through one 8-byte load (dword-aligned: all the hardware asks of a global load)
__device__ __forceinline__ int2 off_pair(const int32_t *__restrict__ off, int64_t r) {
    int2 v;
    __builtin_memcpy(&v, off + r, 8);
    return v;
}

// A lane's four rows: len[j] bytes each (0: a NULL, an empty value, a row past the end), from pool byte `at[j]` (literal) or from `ptr[j]`
// (column; null for a literal).  `vbytes`: the four validity bytes, 1 = the row has a value.
template <bool kCols, bool kSlices>
__device__ __forceinline__ void pick4(const typename TableOf<kSlices>::type &t, int32_t k, const int32_t *__restrict__ sel, const uint8_t *__restrict__ sel_valid, int64_t i0, int64_t n,
                                      uint32_t (&len)[4], uint32_t (&at)[4], const uint8_t *(&ptr)[4], uint32_t *vbytes) {
    int32_t s[4] = {0, 0, 0, 0};
    uint32_t v = 0x01010101u;
    const bool whole = i0 + 4 <= n;
    if (sel) {
        if (whole) {
            const int4 q = *reinterpret_cast<const int4 *>(sel + i0);
            s[0] = q.x; s[1] = q.y; s[2] = q.z; s[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j < n) s[j] = sel[i0 + j];
        }
    }
    if (sel_valid) {
        if (whole) {
            v = *reinterpret_cast<const uint32_t *>(sel_valid + i0);
        } else {
            v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j < n) v |= (uint32_t)(sel_valid[i0 + j] != 0) << (8 * j);
        }
    }
    uint32_t out_v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        bool ok = i0 + j < n && ((v >> (8 * j)) & 0xffu) != 0;
        const uint32_t si = (uint32_t)s[j] < (uint32_t)k ? (uint32_t)s[j] : 0u;
        len[j] = 0;
        at[j] = 0;
        ptr[j] = nullptr;
        if (kCols && t.offsets[si]) {
            const uint8_t *sv = t.valid[si];
            if (ok && sv && !sv[i0 + j]) ok = false;
            if (ok) {
                int2 o;
                bool sliced = false;
                if constexpr (kSlices) {
                    if (t.begin[si]) {
                        o = make_int2(t.begin[si][i0 + j], t.end[si][i0 + j]);
                        sliced = true;
                    }
                }
                if (!sliced) o = off_pair(t.offsets[si], i0 + j);
                len[j] = (uint32_t)(o.y - o.x);
                ptr[j] = t.bytes[si] + (uint32_t)o.x;
            }
        } else if (ok) {
            len[j] = t.lit_len[si];
            at[j] = t.lit_off[si];
        }
        out_v |= (uint32_t)ok << (8 * j);
    }
    *vbytes = out_v;
}

template <bool kCols, bool kSlices>
__global__ __launch_bounds__(kBlock) void textsel_len_kernel(TextSources S, const int32_t *__restrict__ sel, const uint8_t *__restrict__ sel_valid, int64_t n,
                                                             uint32_t *__restrict__ counts, uint8_t *__restrict__ out_valid) {
    __shared__ typename TableOf<kSlices>::type t;
    load_table<kCols, kSlices>(S, t);
    const int64_t i0 = (int64_t)blockIdx.x * kTextTile + (int64_t)threadIdx.x * kRowsPerLane;
    uint32_t len[4], at[4], vb;
    const uint8_t *ptr[4];
    pick4<kCols, kSlices>(t, S.k, sel, sel_valid, i0, n, len, at, ptr, &vb);
    if (out_valid) {
        if (i0 + 4 <= n) {
            *reinterpret_cast<uint32_t *>(out_valid + i0) = vb;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j < n) out_valid[i0 + j] = (uint8_t)((vb >> (8 * j)) & 1u);
        }
    }
    // (a wave's 256 values can come from several columns of almost 2^31 bytes each: summed in 64 bits and saturated, so that a wrapped count can
    // never bring the published total back under the 2^31 bytes the host refuses)
    const uint64_t incl = wave_incl_scan_u64((uint64_t)len[0] + len[1] + len[2] + len[3]);
    if (lane_id() == 63) counts[(size_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)] = incl > 0xffffffffull ? 0xffffffffu : (uint32_t)incl;
}

// `todo` >= 1 bytes into the stage at byte `at`, from the aligned dwords at w on, the first of them `mis` bytes into *w (global memory or the LDS pool:
// one loop).  Up to three bytes bring the destination to a dword boundary, whole dwords follow -- two aligned source dwords funnel-shifted into one
// aligned LDS store; a dword of the stage is written whole only where all four bytes are this value's, so neighbouring values never share a store --,
// up to three bytes end it.  A source dword is read only if it holds a byte of the value.
template <typename Word>
__device__ __forceinline__ void copy_bytes(uint8_t *stage, uint32_t at, const Word *w, uint32_t mis, uint32_t todo) {
    auto few = [&](uint32_t n) {   // n <= 3 bytes, byte by byte
        const uint32_t sh = 8 * (mis & 3u), lo = w[mis >> 2], hi = (mis & 3u) + n > 4u ? w[(mis >> 2) + 1] : 0u;
        const uint32_t v = __funnelshift_r(lo, hi, sh);
        for (uint32_t b = 0; b < n; ++b) stage[at + b] = (uint8_t)(v >> (8 * b));
        at += n;
        mis += n;
        todo -= n;
    };
    const uint32_t head = min((4u - (at & 3u)) & 3u, todo);
    if (head) few(head);
    if (todo >= 4) {
        const Word *q = w + (mis >> 2);
        const uint32_t sh = 8 * (mis & 3u);
        uint32_t lo = *q++;
        for (; todo >= 4; todo -= 4, at += 4, mis += 4) {
            uint32_t v = lo;
            if (sh) {   // (the next dword holds the last of these four bytes)
                const uint32_t hi = *q++;
                v = __funnelshift_r(lo, hi, sh);
                lo = hi;
            } else if (todo >= 5) {
                lo = *q++;
            }
            *reinterpret_cast<uint32_t *>(stage + at) = v;
        }
    }
    if (todo) few(todo);
}

template <bool kCols, bool kSlices>
__global__ __launch_bounds__(kBlock) void textsel_emit_kernel(TextSources S, const int32_t *__restrict__ sel, const uint8_t *__restrict__ sel_valid, int64_t n,
                                                              const uint32_t *__restrict__ counts, const uint64_t *__restrict__ tile_base,
                                                              int32_t *__restrict__ out_off, uint8_t *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[kTextStageBytes];
    __shared__ typename TableOf<kSlices>::type t;
    load_table<kCols, kSlices>(S, t);
    const int wave = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * kTextTile + (int64_t)threadIdx.x * kRowsPerLane;
    uint32_t len[4], at[4], vb;
    const uint8_t *ptr[4];
    pick4<kCols, kSlices>(t, S.k, sel, sel_valid, i0, n, len, at, ptr, &vb);
    const uint32_t mine = len[0] + len[1] + len[2] + len[3];
    const uint4 wc = *reinterpret_cast<const uint4 *>(counts + (size_t)blockIdx.x * kWavesPerBlock);
    const uint32_t tile_bytes = wc.x + wc.y + wc.z + wc.w;
    const uint64_t base = tile_base[blockIdx.x];
    // where the lane's rows start inside the tile: the lower waves' bytes, the lower lanes', the lane's own rows in front
    uint32_t start[4];
    start[0] = (wave > 0 ? wc.x : 0u) + (wave > 1 ? wc.y : 0u) + (wave > 2 ? wc.z : 0u) + wave_incl_scan_u32(mine) - mine;
#pragma unroll
    for (int j = 1; j < 4; ++j) start[j] = start[j - 1] + len[j - 1];
    if (i0 + 4 <= n) {
        stream_store4(out_off + i0, make_uint4((uint32_t)(base + start[0]), (uint32_t)(base + start[1]), (uint32_t)(base + start[2]), (uint32_t)(base + start[3])));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < n) out_off[i0 + j] = (int32_t)(base + start[j]);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out_off[n] = (int32_t)(base + tile_bytes);
    const uint32_t phase = (uint32_t)(base & 15);   // stage byte i holds output byte (base - phase) + i
    const uint32_t end = phase + tile_bytes;
    if (tile_bytes == 0 || end > (uint32_t)kTextStageBytes) return;   // (block-uniform; a tile beyond the stage: textsel_emit_long_kernel writes its bytes)
    uint8_t *gout = out + (base - phase);           // 16-byte aligned
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (len[j] == 0) continue;
        if (kCols && ptr[j]) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(ptr[j]);
            copy_bytes(s_stage, phase + start[j], reinterpret_cast<const uint32_t *>(a & ~uintptr_t(3)), (uint32_t)(a & 3), len[j]);
        } else {
            copy_bytes(s_stage, phase + start[j], t.pool + (at[j] >> 2), at[j] & 3u, len[j]);
        }
    }
    __syncthreads();
    for (uint32_t o = threadIdx.x * 16; o < end; o += kBlock * 16) {
        if (o >= phase && o + 16 <= end) {
            stream_store4(gout + o, *reinterpret_cast<const uint4 *>(s_stage + o));
        } else {   // the tile's first / last chunk is shared with the neighbouring tile: only this tile's bytes
            for (uint32_t c = (o < phase ? phase : o); c < o + 16 && c < end; ++c) gout[c] = s_stage[c];
        }
    }
}

// The bytes of the tiles that do not fit the stage (values of more than 16 bytes on average -- an auction's description -- up to single values of
// any length): the take's chunk-wise emit for long values (utf8_chunks.hpp), over this tile's (address, length) list.  A literal's address lies in
// `pool`, the table's literal pool in global memory.  Offsets are textsel_emit_kernel's.
template <bool kSlices>
__global__ __launch_bounds__(kBlock) void textsel_emit_long_kernel(TextSources S, const uint8_t *__restrict__ pool, const int32_t *__restrict__ sel,
                                                                   const uint8_t *__restrict__ sel_valid, int64_t n, const uint32_t *__restrict__ counts,
                                                                   const uint64_t *__restrict__ tile_base, uint8_t *__restrict__ out) {
    __shared__ uint32_t s_end[kTextTile];
    __shared__ uint64_t s_addr[kTextTile];
    __shared__ uint16_t s_first[kLongMapChunks];
    __shared__ typename TableOf<kSlices>::type t;
    const uint4 wc = *reinterpret_cast<const uint4 *>(counts + (size_t)blockIdx.x * kWavesPerBlock);
    const uint32_t tile_bytes = wc.x + wc.y + wc.z + wc.w;
    const uint64_t base = tile_base[blockIdx.x];
    const uint32_t phase = (uint32_t)(base & 15), end = phase + tile_bytes;
    if (tile_bytes == 0 || end <= (uint32_t)kTextStageBytes) return;   // (block-uniform: the staged kernel's tile)
    load_table<true, kSlices>(S, t);
    const int wave = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * kTextTile + (int64_t)threadIdx.x * kRowsPerLane;
    uint32_t len[4], at[4], vb;
    const uint8_t *ptr[4];
    pick4<true, kSlices>(t, S.k, sel, sel_valid, i0, n, len, at, ptr, &vb);
    const uint32_t mine = len[0] + len[1] + len[2] + len[3];
    uint32_t start[4], index[4];
    start[0] = phase + (wave > 0 ? wc.x : 0u) + (wave > 1 ? wc.y : 0u) + (wave > 2 ? wc.z : 0u) + wave_incl_scan_u32(mine) - mine;
#pragma unroll
    for (int j = 1; j < 4; ++j) start[j] = start[j - 1] + len[j - 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        index[j] = threadIdx.x * kRowsPerLane + j;   // (value index = row order = output order)
        s_end[index[j]] = start[j] + len[j];
        s_addr[index[j]] = ptr[j] ? reinterpret_cast<uintptr_t>(ptr[j]) : reinterpret_cast<uintptr_t>(pool) + at[j];
    }
    utf8_emit_chunks<kTextTile, kRowsPerLane>(s_end, [&](uint32_t v) { return (uintptr_t)s_addr[v]; }, s_first, start, len, index, phase, end, out + (base - phase));
}

// A bare literal of `len` >= 1 bytes for every row: chunk c holds output bytes 16c .. 16c + 15 = the literal from byte (16c mod len) on, over and over
__global__ __launch_bounds__(kBlock) void textsel_fill_kernel(TextSources S, int64_t n, int32_t *__restrict__ out_off, uint8_t *__restrict__ out) {
    __shared__ uint8_t s_lit[kTextMaxLiteralBytes];
    const uint32_t len = S.src[0].lit_len;
    for (uint32_t i = threadIdx.x; i < (len + 3u) / 4u; i += kBlock) reinterpret_cast<uint32_t *>(s_lit)[i] = S.pool[(S.src[0].lit_off >> 2) + i];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kBlock, first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int64_t i = first; i <= n; i += stride) out_off[i] = (int32_t)(i * (int64_t)len);
    const int64_t total = n * (int64_t)len, chunks = (total + 15) / 16;
    for (int64_t c = first; c < chunks; c += stride) {
        uint32_t p = (uint32_t)((c * 16) % (int64_t)len), w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            w[b >> 2] |= (uint32_t)s_lit[p] << (8 * (b & 3));
            p = p + 1 == len ? 0u : p + 1;
        }
        if (c * 16 + 16 <= total) {
            stream_store4(out + c * 16, make_uint4(w[0], w[1], w[2], w[3]));
        } else {
            for (int64_t b = c * 16; b < total; ++b) out[b] = (uint8_t)(w[(b & 15) >> 2] >> (8 * (b & 3)));
        }
    }
}

}  // namespace

namespace flockgpu {

int text_select(flockgpu_ctx *ctx, const char *name, const TextSources &S, const int32_t *sel, const uint8_t *sel_valid, int64_t rows, DevColumn *out) {
    const std::string base = name;
    *out = DevColumn{};
    out->type = ColType::UTF8;
    out->nullable = true;
    if (S.k < 0 || S.k > kTextMaxSources) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: 0 to %d text sources", name, kTextMaxSources);
    if (rows >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than 2^31 rows", name);
    const int64_t n = std::max<int64_t>(rows, 0);
    int32_t *o_off = nullptr;
    uint8_t *o_b = nullptr, *o_v = nullptr;
    FG_TRY(arena_get_t(ctx, (base + ".off").c_str(), (size_t)n + 4, &o_off));
    out->offsets = o_off;
    bool nulls = sel_valid != nullptr || S.k == 0;
    for (int i = 0; i < S.k; ++i) nulls = nulls || (S.src[i].offsets && S.src[i].valid);
    if (nulls) FG_TRY(arena_get_t(ctx, (base + ".valid").c_str(), (size_t)n + 16, &o_v));
    out->valid = o_v;
    if (n == 0 || S.k == 0) {   // no row, or no source: every row NULL
        FG_HIP(ctx, hipMemsetAsync(o_off, 0, sizeof(int32_t) * ((size_t)n + 1), ctx->stream));
        if (o_v && n) FG_HIP(ctx, hipMemsetAsync(o_v, 0, (size_t)n, ctx->stream));
        FG_TRY(arena_get_t(ctx, (base + ".bytes").c_str(), 16, &o_b));
        out->values = o_b;
        return FLOCKGPU_OK;
    }
    if (!sel && !sel_valid && S.k == 1 && !S.src[0].offsets) {   // a bare literal: one fill
        const uint64_t total = (uint64_t)n * S.src[0].lit_len;
        if (total > 0x7fffffffull) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: Utf8 column exceeds 2^31 bytes", name);
        FG_TRY(arena_get_t(ctx, (base + ".bytes").c_str(), (size_t)total + 16, &o_b));
        out->values = o_b;
        out->bytes = (int64_t)total;
        if (S.src[0].lit_len == 0) {
            FG_HIP(ctx, hipMemsetAsync(o_off, 0, sizeof(int32_t) * ((size_t)n + 1), ctx->stream));
            return FLOCKGPU_OK;
        }
        const unsigned grid = (unsigned)std::min<int64_t>(div_up(std::max<int64_t>(n + 1, (int64_t)(total + 15) / 16), kBlock), (int64_t)ctx->num_cus * 16);
        {
            LaunchScope ls(ctx, "textsel_fill_kernel");
            hipLaunchKernelGGL(textsel_fill_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, S, n, o_off, o_b);
        }
        return check_launch(ctx, "textsel_fill_kernel");
    }
    const int64_t tiles = div_up(n, kTextTile);
    uint32_t *counts = nullptr;
    uint64_t *tile_base = nullptr, *h_total = nullptr;
    FG_TRY(arena_get_t(ctx, (base + ".counts").c_str(), (size_t)tiles * kWavesPerBlock, &counts));
    FG_TRY(arena_get_t(ctx, (base + ".base").c_str(), (size_t)tiles + 1, &tile_base));
    FG_TRY(pinned_get_t(ctx, (base + ".total").c_str(), 1, &h_total));
    *h_total = 0;
    const bool cols = S.n_cols > 0, slices = S.n_slices > 0;   // (a table without a slice source takes the instances it always took)
    {
        LaunchScope ls(ctx, "textsel_len_kernel");
        if (slices) hipLaunchKernelGGL((textsel_len_kernel<true, true>), dim3((unsigned)tiles), dim3(kBlock), 0, ctx->stream, S, sel, sel_valid, n, counts, o_v);
        else if (cols) hipLaunchKernelGGL((textsel_len_kernel<true, false>), dim3((unsigned)tiles), dim3(kBlock), 0, ctx->stream, S, sel, sel_valid, n, counts, o_v);
        else hipLaunchKernelGGL((textsel_len_kernel<false, false>), dim3((unsigned)tiles), dim3(kBlock), 0, ctx->stream, S, sel, sel_valid, n, counts, o_v);
    }
    FG_TRY(check_launch(ctx, "textsel_len_kernel"));
    FG_TRY(launch_tile_scan(ctx, counts, (int32_t)tiles, tile_base, nullptr, 0, nullptr));
    FG_TRY(publish_words(ctx, PublishList().add(h_total, tile_base + tiles, 2)));
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t total = *h_total;
    if (total > 0x7fffffffull) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: Utf8 column exceeds 2^31 bytes", name);
    FG_TRY(arena_get_t(ctx, (base + ".bytes").c_str(), (size_t)total + 16, &o_b));
    {
        LaunchScope ls(ctx, "textsel_emit_kernel");
        if (slices) hipLaunchKernelGGL((textsel_emit_kernel<true, true>), dim3((unsigned)tiles), dim3(kBlock), 0, ctx->stream, S, sel, sel_valid, n, counts, tile_base, o_off, o_b);
        else if (cols) hipLaunchKernelGGL((textsel_emit_kernel<true, false>), dim3((unsigned)tiles), dim3(kBlock), 0, ctx->stream, S, sel, sel_valid, n, counts, tile_base, o_off, o_b);
        else hipLaunchKernelGGL((textsel_emit_kernel<false, false>), dim3((unsigned)tiles), dim3(kBlock), 0, ctx->stream, S, sel, sel_valid, n, counts, tile_base, o_off, o_b);
    }
    FG_TRY(check_launch(ctx, "textsel_emit_kernel"));
    // tiles beyond the stage: possible with a column source, or with literals of more than a stage per tile
    uint32_t longest = 0;
    for (int i = 0; i < S.k; ++i) longest = std::max(longest, S.src[i].lit_len);
    if (total + 15 > (uint64_t)kTextStageBytes && (cols || (uint64_t)longest * kTextTile + 15 > (uint64_t)kTextStageBytes)) {
        uint8_t *d_pool = nullptr, *h_pool = nullptr;
        FG_TRY(arena_get_t(ctx, (base + ".pool").c_str(), sizeof(S.pool) + 32, &d_pool));
        FG_TRY(pinned_get_t(ctx, (base + ".pool").c_str(), sizeof(S.pool), &h_pool));
        std::memcpy(h_pool, S.pool, sizeof(S.pool));   // (the stream is idle: the wait above)
        FG_HIP(ctx, hipMemcpyAsync(d_pool, h_pool, sizeof(S.pool), hipMemcpyHostToDevice, ctx->stream));
        {
            LaunchScope ls(ctx, "textsel_emit_long_kernel");
            if (slices) hipLaunchKernelGGL(textsel_emit_long_kernel<true>, dim3((unsigned)tiles), dim3(kBlock), 0, ctx->stream, S, d_pool, sel, sel_valid, n, counts, tile_base, o_b);
            else hipLaunchKernelGGL(textsel_emit_long_kernel<false>, dim3((unsigned)tiles), dim3(kBlock), 0, ctx->stream, S, d_pool, sel, sel_valid, n, counts, tile_base, o_b);
        }
        FG_TRY(check_launch(ctx, "textsel_emit_long_kernel"));
    }
    out->values = o_b;
    out->bytes = (int64_t)total;
    return FLOCKGPU_OK;
}

}  // namespace flockgpu
