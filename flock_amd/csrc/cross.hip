// CrossJoinExec's column kernels (cross.hpp): repeat and tile of fixed-width values, validity bytes, Utf8 offsets and Utf8 bytes.
// Every index is checked against the output's length; a source index is taken only for an output element that exists, so no lane reads behind
// src[rows - 1] (Utf8: behind off[rows]).  Output buffers are 16-byte aligned (arena buffers are) and asked for with 16 bytes of slack.
#include <algorithm>
#include <string>

#include "cross.hpp"
#include "utf8_chunks.hpp"

using namespace flockgpu;

namespace {

constexpr int kChunksPerLane = kCrossTileChunks / kBlock;   // 4
static_assert(kCrossTileChunks % kBlock == 0, "a workgroup's chunks are whole rounds of its lanes");
static_assert(kCrossTextTile == 4 * kBlock, "cross_repeat_bytes_kernel: four output values per lane");

template <typename T>
__device__ __forceinline__ uint4 pack16(const T (&v)[16 / sizeof(T)]) {
    uint4 q;
    __builtin_memcpy(&q, v, 16);
    return q;
}

// out[e] = src[e / R] (repeat) or src[e % R] (tile) for e < n_out; mR.d = R.  One 16-byte chunk of the output per lane and round.
template <typename T, bool kTile>
__device__ __forceinline__ void cross_fixed(const T *__restrict__ src, UMod32 mR, uint32_t n_out, T *__restrict__ out) {
    constexpr uint32_t E = 16 / sizeof(T);
    const uint32_t chunks = (n_out + E - 1) / E;   // (n_out < 2^31)
    const uint32_t R = mR.d;
#pragma unroll
    for (int k = 0; k < kChunksPerLane; ++k) {
        const uint32_t c = blockIdx.x * (uint32_t)kCrossTileChunks + (uint32_t)k * kBlock + threadIdx.x;
        if (c >= chunks) return;
        const uint32_t e0 = c * E;
        uint32_t q, r;
        cross_divmod(e0, mR, &q, &r);
        T v[E], cur = T(0);
#pragma unroll
        for (uint32_t j = 0; j < E; ++j) {
            const bool live = e0 + j < n_out;
            if (kTile) {
                cur = live ? src[r] : T(0);
            } else if (live && (j == 0 || r == 0)) {   // (the source row changes where the remainder wraps)
                cur = src[q];
            }
            v[j] = cur;
            if (++r == R) { r = 0; ++q; }
        }
        if (e0 + E <= n_out) {
            stream_store4(out + e0, pack16<T>(v));
        } else {
#pragma unroll
            for (uint32_t j = 0; j < E; ++j)
                if (e0 + j < n_out) out[e0 + j] = v[j];
        }
    }
}
template <typename T>
__global__ __launch_bounds__(kBlock) void cross_repeat_kernel(const T *__restrict__ src, UMod32 mR, uint32_t n_out, T *__restrict__ out) {
    cross_fixed<T, false>(src, mR, n_out, out);
}
template <typename T>
__global__ __launch_bounds__(kBlock) void cross_tile_kernel(const T *__restrict__ src, UMod32 mR, uint32_t n_out, T *__restrict__ out) {
    cross_fixed<T, true>(src, mR, n_out, out);
}

// Utf8 offsets, n_out + 1 of them (entry n_out = the byte total), four per lane as one aligned 16-byte store.  mT.d = `times`.
//   repeat (kTile false): entry i * times + j = times * off[i] + j * (off[i + 1] - off[i])   (the last entry: i = rows, j = 0 -- off[rows + 1] is not read)
//   tile:                 entry i * rows + j  = i * total + off[j]                            (mT.d = rows here; the last entry: i = times, j = 0)
template <bool kTile>
__global__ __launch_bounds__(kBlock) void cross_offsets_kernel(const int32_t *__restrict__ off, UMod32 mT, uint64_t total, uint32_t n_out, int32_t *__restrict__ out_off) {
    const uint32_t entries = n_out + 1, chunks = (entries + 3) / 4, D = mT.d;
#pragma unroll
    for (int k = 0; k < kChunksPerLane; ++k) {
        const uint32_t c = blockIdx.x * (uint32_t)kCrossTileChunks + (uint32_t)k * kBlock + threadIdx.x;
        if (c >= chunks) return;
        const uint32_t e0 = c * 4;
        uint32_t q, r;
        cross_divmod(e0, mT, &q, &r);
        uint32_t v[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            v[j] = 0;
            if (e0 + j < entries) {
                if (kTile) {
                    v[j] = (uint32_t)cross_tile_offset(total, q, (uint64_t)(uint32_t)off[r]);
                } else {
                    const uint64_t o = (uint64_t)(uint32_t)off[q];
                    v[j] = (uint32_t)cross_repeat_offset(D, r, o, r ? (uint64_t)(uint32_t)off[q + 1] - o : 0);
                }
            }
            if (++r == D) { r = 0; ++q; }
        }
        if (e0 + 4 <= entries) {
            stream_store4(out_off + e0, make_uint4(v[0], v[1], v[2], v[3]));
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (e0 + j < entries) out_off[e0 + j] = (int32_t)v[j];
        }
    }
}

// out[b] = src[b % total] for b < out_bytes (total >= 1, mB.d = total): the source bytes over and over.  A chunk that lies inside one copy reads the
// aligned dwords that hold its sixteen bytes (the last of them ends before src + total + 3: source buffers carry 16 bytes of slack) and
// funnel-shifts them; the chunk that wraps -- every chunk when total < 16 -- goes byte by byte.
__global__ __launch_bounds__(kBlock) void cross_tile_bytes_kernel(const uint8_t *__restrict__ src, UMod32 mB, uint32_t out_bytes, uint8_t *__restrict__ out) {
    const uint32_t chunks = (out_bytes + 15) / 16, total = mB.d;
#pragma unroll
    for (int k = 0; k < kChunksPerLane; ++k) {
        const uint32_t c = blockIdx.x * (uint32_t)kCrossTileChunks + (uint32_t)k * kBlock + threadIdx.x;
        if (c >= chunks) return;
        const uint32_t b0 = c * 16;
        uint32_t p = umod32_apply(b0, mB);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (p + 16 <= total) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(src + p);
            const uint32_t *q = reinterpret_cast<const uint32_t *>(a & ~uintptr_t(3));
            const uint32_t sh = 8 * (uint32_t)(a & 3);
            uint32_t d[5];
#pragma unroll
            for (int i = 0; i < 4; ++i) d[i] = q[i];
            d[4] = sh ? q[4] : 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = sh ? __funnelshift_r(d[i], d[i + 1], sh) : d[i];
        } else {
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                w[b >> 2] |= (uint32_t)src[p] << (8 * (b & 3));
                p = p + 1 == total ? 0u : p + 1;
            }
        }
        if (b0 + 16 <= out_bytes) {
            stream_store4(out + b0, make_uint4(w[0], w[1], w[2], w[3]));
        } else {
            for (uint32_t b = b0; b < out_bytes; ++b) out[b] = (uint8_t)(w[(b & 15) >> 2] >> (8 * (b & 3)));
        }
    }
}

// The bytes of a repeated Utf8 column: output value v = i * times + j holds source value i.  A workgroup owns kCrossTextTile consecutive OUTPUT values;
// where they start is the closed form of cross_offsets_kernel (no length pass, no scan), and the bytes go out through the take's chunk-wise emit
// (utf8_chunks.hpp): every lane builds whole 16-byte chunks of the output from aligned 16-byte source chunks.
__global__ __launch_bounds__(kBlock) void cross_repeat_bytes_kernel(const int32_t *__restrict__ off, const uint8_t *__restrict__ src, UMod32 mT, uint32_t n_out,
                                                                    uint32_t out_bytes, uint8_t *__restrict__ out) {
    __shared__ uint32_t s_end[kCrossTextTile];
    __shared__ uint64_t s_addr[kCrossTextTile];
    __shared__ uint16_t s_first[kLongMapChunks];
    const uint32_t D = mT.d;
    auto start_of = [&](uint32_t v) -> uint64_t {   // first byte of output value v (v <= n_out)
        uint32_t q, r;
        cross_divmod(v, mT, &q, &r);
        const uint64_t o = (uint64_t)(uint32_t)off[q];
        return cross_repeat_offset(D, r, o, r ? (uint64_t)(uint32_t)off[q + 1] - o : 0);
    };
    const uint32_t v0 = blockIdx.x * (uint32_t)kCrossTextTile;
    const uint32_t v1 = min(v0 + (uint32_t)kCrossTextTile, n_out);
    const uint64_t base = start_of(v0);
    const uint32_t tile_bytes = (uint32_t)(start_of(v1) - base);
    // (block-uniform; a tile that would end behind the bytes the host sized the buffer for -- offsets that disagree with the column's byte total -- writes nothing)
    if (tile_bytes == 0 || base + tile_bytes > out_bytes) return;
    const uint32_t phase = (uint32_t)(base & 15), end = phase + tile_bytes;
    uint32_t start[4], len[4], index[4];
    uint32_t q, r;
    cross_divmod(v0 + threadIdx.x * 4u, mT, &q, &r);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t v = v0 + threadIdx.x * 4u + j;
        index[j] = threadIdx.x * 4u + j;
        start[j] = end;
        len[j] = 0;
        uint64_t addr = reinterpret_cast<uintptr_t>(src);
        if (v < n_out) {
            const uint32_t o = (uint32_t)off[q], l = (uint32_t)off[q + 1] - o;
            start[j] = phase + (uint32_t)(cross_repeat_offset(D, r, o, l) - base);
            len[j] = l;
            addr += o;
        }
        s_end[index[j]] = start[j] + len[j];
        s_addr[index[j]] = addr;
        if (++r == D) { r = 0; ++q; }
    }
    utf8_emit_chunks<kCrossTextTile, 4>(s_end, [&](uint32_t v) { return (uintptr_t)s_addr[v]; }, s_first, start, len, index, phase, end, out + (base - phase));
}

template <typename T>
int launch_fixed(flockgpu_ctx *ctx, bool tile, bool fill, const void *src, uint32_t divisor, int64_t n_out, void *out) {
    if (n_out <= 0) return FLOCKGPU_OK;
    const UMod32 m = umod32_make(divisor);
    const int64_t chunks = div_up(n_out, (int64_t)(16 / sizeof(T)));
    const unsigned grid = (unsigned)div_up(chunks, kCrossTileChunks);
    const char *label = tile ? "cross_tile_kernel" : fill ? "cross_fill_kernel" : "cross_repeat_kernel";
    {
        LaunchScope ls(ctx, label);
        if (tile) hipLaunchKernelGGL(cross_tile_kernel<T>, dim3(grid), dim3(kBlock), 0, ctx->stream, static_cast<const T *>(src), m, (uint32_t)n_out, static_cast<T *>(out));
        else hipLaunchKernelGGL(cross_repeat_kernel<T>, dim3(grid), dim3(kBlock), 0, ctx->stream, static_cast<const T *>(src), m, (uint32_t)n_out, static_cast<T *>(out));
    }
    return check_launch(ctx, label);
}

// repeat: `rows` source values, `times` times each; tile: `rows` source values as a whole, `times` times over.  A tile of ONE row is the repeat of it.
int cross_column(flockgpu_ctx *ctx, const char *name, const DevColumn &src, int64_t rows, int64_t times, bool tile, DevColumn *out) {
    const std::string base = name;
    if (tile && rows == 1) tile = false;
    int64_t n = 0, out_bytes = 0;
    if (!cross_rows_ok(rows, times, &n)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: %lld x %lld rows: more than 2^31 rows", name, (long long)rows, (long long)times);
    const bool utf8 = src.type == ColType::UTF8;
    if (utf8 && n > 0 && !cross_bytes_ok(src.bytes, times, &out_bytes)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: Utf8 column exceeds 2^31 bytes", name);
    *out = src;
    out->valid = nullptr;
    out->offsets = nullptr;
    out->bytes = 0;
    // the divisor: a repeat steps to the next source row every `times` outputs, a tile wraps every `rows`
    const uint32_t divisor = (uint32_t)std::max<int64_t>(tile ? rows : times, 1);
    const bool fill = !tile && rows == 1;
    if (src.valid) {
        uint8_t *v = nullptr;
        FG_TRY(arena_get_t(ctx, (base + ".valid").c_str(), (size_t)n + 16, &v));
        FG_TRY(launch_fixed<uint8_t>(ctx, tile, fill, src.valid, divisor, n, v));
        out->valid = v;
    }
    if (!utf8) {
        void *pv = nullptr;
        const size_t w = col_width(src.type);
        FG_TRY(arena_get(ctx, (base + ".val").c_str(), (size_t)n * w + 16, &pv));
        if (w == 4) FG_TRY(launch_fixed<uint32_t>(ctx, tile, fill, src.values, divisor, n, pv));
        else FG_TRY(launch_fixed<uint64_t>(ctx, tile, fill, src.values, divisor, n, pv));
        out->values = pv;
        return FLOCKGPU_OK;
    }
    int32_t *o_off = nullptr;
    uint8_t *o_b = nullptr;
    FG_TRY(arena_get_t(ctx, (base + ".off").c_str(), (size_t)n + 4, &o_off));
    FG_TRY(arena_get_t(ctx, (base + ".bytes").c_str(), (size_t)out_bytes + 16, &o_b));
    out->offsets = o_off;
    out->values = o_b;
    out->bytes = out_bytes;
    if (n == 0) {
        FG_HIP(ctx, hipMemsetAsync(o_off, 0, sizeof(int32_t), ctx->stream));
        return FLOCKGPU_OK;
    }
    {
        const UMod32 m = umod32_make(divisor);
        const unsigned grid = (unsigned)div_up(div_up(n + 1, 4), kCrossTileChunks);
        LaunchScope ls(ctx, "cross_offsets_kernel");
        if (tile) hipLaunchKernelGGL(cross_offsets_kernel<true>, dim3(grid), dim3(kBlock), 0, ctx->stream, src.offsets, m, (uint64_t)src.bytes, (uint32_t)n, o_off);
        else hipLaunchKernelGGL(cross_offsets_kernel<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, src.offsets, m, (uint64_t)src.bytes, (uint32_t)n, o_off);
    }
    FG_TRY(check_launch(ctx, "cross_offsets_kernel"));
    if (out_bytes == 0) return FLOCKGPU_OK;
    if (tile) {
        const UMod32 mb = umod32_make((uint32_t)src.bytes);
        const unsigned grid = (unsigned)div_up(div_up(out_bytes, 16), kCrossTileChunks);
        {
            LaunchScope ls(ctx, "cross_tile_bytes_kernel");
            hipLaunchKernelGGL(cross_tile_bytes_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, static_cast<const uint8_t *>(src.values), mb, (uint32_t)out_bytes, o_b);
        }
        return check_launch(ctx, "cross_tile_bytes_kernel");
    }
    const UMod32 m = umod32_make(divisor);
    const unsigned grid = (unsigned)div_up(n, kCrossTextTile);
    const char *label = fill ? "cross_fill_bytes_kernel" : "cross_repeat_bytes_kernel";
    {
        LaunchScope ls(ctx, label);
        hipLaunchKernelGGL(cross_repeat_bytes_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, src.offsets, static_cast<const uint8_t *>(src.values), m, (uint32_t)n, (uint32_t)out_bytes, o_b);
    }
    return check_launch(ctx, label);
}

}  // namespace

namespace flockgpu {

int cross_repeat(flockgpu_ctx *ctx, const char *name, const DevColumn &src, int64_t rows, int64_t times, DevColumn *out) {
    return cross_column(ctx, name, src, rows, times, false, out);
}
int cross_tile(flockgpu_ctx *ctx, const char *name, const DevColumn &src, int64_t rows, int64_t times, DevColumn *out) {
    return cross_column(ctx, name, src, rows, times, true, out);
}

}  // namespace flockgpu
