// CAST(x AS Utf8) of an Int32 / Int64 / UInt64 / Timestamp(ms) column (numtext.hpp A-NT1..A-NT7): a fixed-width column -> an ordinary Utf8 column.
// The shape is text_select's (textsel.hip) -- a length pass, the tile scan, an emit pass over tiles of kTextTile rows, FOUR CONSECUTIVE rows per lane --
// but a row's bytes are COMPUTED, not copied, and there are at most 23 of them, so a tile's bytes are bounded statically: the stage holds any tile and
// there is no path for long values.
//   numtext_len_kernel    per row the byte count (digit count + sign; 19 or 23 for a timestamp) -> one count per wave for the tile scan (scan.hpp); the
//                         result's validity bytes where a NULL can occur (the input has NULLs, or a try_cast_expr meets a timestamp outside the years
//                         0000..9999); a flag word when a cast_expr meets such a timestamp, which the host reads with the byte total.
//   numtext_emit_kernel   offsets: one aligned 16-byte store per lane.  Bytes: a lane formats a row in registers (numtext.hpp: the text as 3 / 5 / 6
//                         dwords), shifts the words so that they line up with the stage's dwords at the row's position -- a word shift by select, a
//                         byte shift by funnel shift -- and writes ALIGNED dwords into the LDS stage, the row's first and last up to three bytes byte
//                         by byte (a dword is written whole only where all four bytes are this row's; a misaligned LDS access costs 6x on gfx950,
//                         README round 3).  The stage leaves as aligned 16-byte non-temporal stores; the tile's first and last chunk, which it shares
//                         with its neighbours, byte by byte.  Where a byte lands depends on the scanned offsets alone: not on batching or grid shape.
// Every row index is checked against `rows`; a tile writes output bytes [tile_base, tile_base + tile bytes) only.
#include <algorithm>

#include "gather.hpp"
#include "scan.hpp"
#include "textsel.hpp"

using namespace flockgpu;

namespace {

constexpr int kRowsPerLane = kTextTile / kBlock;   // 4
static_assert(kRowsPerLane == 4, "a lane's rows are one 16-byte load of 32-bit values and one 16-byte offsets store");

constexpr uint32_t kErrRange = 1u;

// the stage: a tile of the longest rows, behind up to 15 bytes of phase, in whole 16-byte chunks
constexpr int stage_bytes(NumTextKind k) { return (kTextTile * numtext_max_len(k) + 15 + 15) / 16 * 16; }

template <NumTextKind K> struct ValueOf { using type = int64_t; };
template <> struct ValueOf<NumTextKind::I32> { using type = int32_t; };
template <> struct ValueOf<NumTextKind::U64> { using type = uint64_t; };

// A lane's four values and which of them are there (bit j: row i0 + j exists and is not NULL).  `vec`: the column starts on a 16-byte boundary
// (its validity bytes on a 4-byte one): whole groups of four arrive as 16-byte loads.
template <NumTextKind K>
__device__ __forceinline__ uint32_t load4(const void *__restrict__ values, const uint8_t *__restrict__ valid, int64_t i0, int64_t n, bool vec,
                                          typename ValueOf<K>::type (&v)[4]) {
    using T = typename ValueOf<K>::type;
    const T *col = static_cast<const T *>(values);
    uint32_t ok = 0;
    if (vec && i0 + 4 <= n) {
        if constexpr (sizeof(T) == 4) {
            const int4 q = *reinterpret_cast<const int4 *>(col + i0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            const uint4 a = *reinterpret_cast<const uint4 *>(col + i0), b = *reinterpret_cast<const uint4 *>(col + i0 + 2);
            v[0] = (T)((uint64_t)a.x | ((uint64_t)a.y << 32));
            v[1] = (T)((uint64_t)a.z | ((uint64_t)a.w << 32));
            v[2] = (T)((uint64_t)b.x | ((uint64_t)b.y << 32));
            v[3] = (T)((uint64_t)b.z | ((uint64_t)b.w << 32));
        }
        ok = 15u;
        if (valid) {
            const uint32_t m = *reinterpret_cast<const uint32_t *>(valid + i0);
            ok = ((m & 0xffu) ? 1u : 0u) | ((m & 0xff00u) ? 2u : 0u) | ((m & 0xff0000u) ? 4u : 0u) | ((m & 0xff000000u) ? 8u : 0u);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = 0;
            if (i0 + j < n) {
                v[j] = col[i0 + j];
                if (!valid || valid[i0 + j]) ok |= 1u << j;
            }
        }
    }
    return ok;
}

// the byte count of a value (a timestamp: in range)
template <NumTextKind K>
__device__ __forceinline__ uint32_t length_of(typename ValueOf<K>::type v) {
    if constexpr (K == NumTextKind::I32) return numtext::digits10_u32(v < 0 ? 0u - (uint32_t)v : (uint32_t)v) + (v < 0 ? 1u : 0u);
    else if constexpr (K == NumTextKind::I64) return numtext::digits10_u64(v < 0 ? 0ull - (uint64_t)v : (uint64_t)v) + (v < 0 ? 1u : 0u);
    else if constexpr (K == NumTextKind::U64) return numtext::digits10_u64(v);
    else return numtext_ts_len(v);
}
template <NumTextKind K>
__device__ __forceinline__ NumText<numtext_words(K)> format(typename ValueOf<K>::type v) {
    if constexpr (K == NumTextKind::I32) return numtext_i32(v);
    else if constexpr (K == NumTextKind::I64) return numtext_i64(v);
    else if constexpr (K == NumTextKind::U64) return numtext_u64(v, false);
    else return numtext_ts(v);
}

// The four lengths (0: a NULL, a row past the end, a timestamp out of range); *ok loses the timestamps out of range; returns whether there was one.
template <NumTextKind K>
__device__ __forceinline__ bool lengths4(const typename ValueOf<K>::type (&v)[4], uint32_t *ok, uint32_t (&len)[4]) {
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        len[j] = 0;
        if (!((*ok >> j) & 1u)) continue;
        if constexpr (K == NumTextKind::TS) {
            if (!numtext_ts_in_range(v[j])) {
                bad = true;
                *ok &= ~(1u << j);
                continue;
            }
        }
        len[j] = length_of<K>(v[j]);
    }
    return bad;
}

template <NumTextKind K>
__global__ __launch_bounds__(kBlock) void numtext_len_kernel(const void *__restrict__ values, const uint8_t *__restrict__ valid, int64_t n, int32_t vec, int32_t try_cast,
                                                             uint32_t *__restrict__ counts, uint8_t *__restrict__ out_valid, uint32_t *__restrict__ err) {
    const int64_t i0 = (int64_t)blockIdx.x * kTextTile + (int64_t)threadIdx.x * kRowsPerLane;
    typename ValueOf<K>::type v[4];
    uint32_t ok = load4<K>(values, valid, i0, n, vec != 0, v), len[4];
    const bool bad = lengths4<K>(v, &ok, len);
    if (bad && !try_cast) atomicOr(err, kErrRange);
    if (out_valid) {
        if (i0 + 4 <= n) {
            *reinterpret_cast<uint32_t *>(out_valid + i0) = (ok & 1u) | ((ok & 2u) << 7) | ((ok & 4u) << 14) | ((ok & 8u) << 21);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j < n) out_valid[i0 + j] = (uint8_t)((ok >> j) & 1u);
        }
    }
    const uint32_t incl = wave_incl_scan_u32(len[0] + len[1] + len[2] + len[3]);   // (a wave's 256 rows: at most 5888 bytes)
    if (lane_id() == 63) counts[(size_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)] = incl;
}

template <NumTextKind K>
__global__ __launch_bounds__(kBlock) void numtext_emit_kernel(const void *__restrict__ values, const uint8_t *__restrict__ valid, int64_t n, int32_t vec,
                                                              const uint32_t *__restrict__ counts, const uint64_t *__restrict__ tile_base,
                                                              int32_t *__restrict__ out_off, uint8_t *__restrict__ out) {
    constexpr int kStage = stage_bytes(K), kWords = numtext_words(K);
    constexpr int kMaxShift = K == NumTextKind::TS ? 1 : kWords;   // (a timestamp's text begins at byte 0 of its words: a shift of no or one word)
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[kStage];
    const int wave = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * kTextTile + (int64_t)threadIdx.x * kRowsPerLane;
    typename ValueOf<K>::type v[4];
    uint32_t ok = load4<K>(values, valid, i0, n, vec != 0, v), len[4];
    lengths4<K>(v, &ok, len);
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
    if (tile_bytes == 0 || end > (uint32_t)kStage) return;   // (block-uniform; the second cannot be: a tile holds at most kTextTile * the longest text)
    uint8_t *gout = out + (base - phase);           // 16-byte aligned
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (len[j] == 0) continue;
        numtext_place<kWords, kMaxShift>(s_stage, phase + start[j], format<K>(v[j]));
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

template <NumTextKind K>
void launch_len(flockgpu_ctx *ctx, unsigned tiles, const DevColumn &in, int64_t n, bool vec, bool try_cast, uint32_t *counts, uint8_t *o_v, uint32_t *d_err) {
    hipLaunchKernelGGL(numtext_len_kernel<K>, dim3(tiles), dim3(kBlock), 0, ctx->stream, in.values, in.valid, n, (int32_t)vec, (int32_t)try_cast, counts, o_v, d_err);
}
template <NumTextKind K>
void launch_emit(flockgpu_ctx *ctx, unsigned tiles, const DevColumn &in, int64_t n, bool vec, const uint32_t *counts, const uint64_t *tile_base, int32_t *o_off, uint8_t *o_b) {
    hipLaunchKernelGGL(numtext_emit_kernel<K>, dim3(tiles), dim3(kBlock), 0, ctx->stream, in.values, in.valid, n, (int32_t)vec, counts, tile_base, o_off, o_b);
}

}  // namespace

namespace flockgpu {

int num_to_text(flockgpu_ctx *ctx, const char *name, const DevColumn &in, int64_t rows, bool try_cast, const char *who, DevColumn *out) {
    const std::string base = name;
    *out = DevColumn{};
    out->type = ColType::UTF8;
    out->nullable = true;
    if (in.type != ColType::I32 && in.type != ColType::I64 && in.type != ColType::U64) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: %s to Utf8 of a column that is neither an integer nor a Timestamp(ms)", name, who);
    if (rows >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than 2^31 rows", name);
    const NumTextKind kind = in.type == ColType::I32 ? NumTextKind::I32 : in.type == ColType::U64 ? NumTextKind::U64 : in.is_ts ? NumTextKind::TS : NumTextKind::I64;
    const int64_t n = std::max<int64_t>(rows, 0);
    int32_t *o_off = nullptr;
    uint8_t *o_b = nullptr, *o_v = nullptr;
    FG_TRY(arena_get_t(ctx, (base + ".off").c_str(), (size_t)n + 4, &o_off));
    out->offsets = o_off;
    const bool range = kind == NumTextKind::TS;   // a timestamp outside the years 0000..9999: NULL under try_cast_expr, the call's failure under cast_expr
    const bool nulls = in.valid != nullptr || in.all_null || (range && try_cast);
    if (nulls) FG_TRY(arena_get_t(ctx, (base + ".valid").c_str(), (size_t)n + 16, &o_v));
    out->valid = o_v;
    if (n == 0 || in.all_null || !in.values) {   // no row, or no value: every row NULL
        FG_HIP(ctx, hipMemsetAsync(o_off, 0, sizeof(int32_t) * ((size_t)n + 1), ctx->stream));
        if (o_v && n) FG_HIP(ctx, hipMemsetAsync(o_v, 0, (size_t)n, ctx->stream));
        FG_TRY(arena_get_t(ctx, (base + ".bytes").c_str(), 16, &o_b));
        out->values = o_b;
        if (n && !in.all_null) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: %s to Utf8 of a column that was not materialised", name, who);
        return FLOCKGPU_OK;
    }
    const int64_t tiles = div_up(n, kTextTile);
    uint32_t *counts = nullptr, *d_err = nullptr, *h_err = nullptr;
    uint64_t *tile_base = nullptr, *h_total = nullptr;
    FG_TRY(arena_get_t(ctx, (base + ".counts").c_str(), (size_t)tiles * kWavesPerBlock, &counts));
    FG_TRY(arena_get_t(ctx, (base + ".base").c_str(), (size_t)tiles + 1, &tile_base));
    FG_TRY(arena_get_t(ctx, (base + ".err").c_str(), 4, &d_err));
    FG_TRY(pinned_get_t(ctx, (base + ".total").c_str(), 1, &h_total));
    FG_TRY(pinned_get_t(ctx, (base + ".err").c_str(), 4, &h_err));
    *h_total = 0;
    *h_err = 0;
    const bool flagged = range && !try_cast;
    if (flagged) FG_TRY(fill_words(ctx, FillList().add(d_err, 0u, 1)));
    const bool vec = (reinterpret_cast<uintptr_t>(in.values) & 15u) == 0 && (reinterpret_cast<uintptr_t>(in.valid) & 3u) == 0;
    {
        LaunchScope ls(ctx, "numtext_len_kernel");
        switch (kind) {
            case NumTextKind::I32: launch_len<NumTextKind::I32>(ctx, (unsigned)tiles, in, n, vec, try_cast, counts, o_v, d_err); break;
            case NumTextKind::I64: launch_len<NumTextKind::I64>(ctx, (unsigned)tiles, in, n, vec, try_cast, counts, o_v, d_err); break;
            case NumTextKind::U64: launch_len<NumTextKind::U64>(ctx, (unsigned)tiles, in, n, vec, try_cast, counts, o_v, d_err); break;
            case NumTextKind::TS: launch_len<NumTextKind::TS>(ctx, (unsigned)tiles, in, n, vec, try_cast, counts, o_v, d_err); break;
        }
    }
    FG_TRY(check_launch(ctx, "numtext_len_kernel"));
    FG_TRY(launch_tile_scan(ctx, counts, (int32_t)tiles, tile_base, nullptr, 0, nullptr));
    PublishList pub;
    pub.add(h_total, tile_base + tiles, 2);
    if (flagged) pub.add(h_err, d_err, 1);   // (the flag word travels with the byte total: no wait of its own)
    FG_TRY(publish_words(ctx, pub));
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (flagged && (*h_err & kErrRange)) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: %s: a Timestamp(ms) outside the years 0000 to 9999 has no Utf8 form (try_cast_expr gives NULL there)", name, who);
    const uint64_t total = *h_total;
    if (total > 0x7fffffffull) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: Utf8 column exceeds 2^31 bytes", name);
    FG_TRY(arena_get_t(ctx, (base + ".bytes").c_str(), (size_t)total + 16, &o_b));
    {
        LaunchScope ls(ctx, "numtext_emit_kernel");
        switch (kind) {
            case NumTextKind::I32: launch_emit<NumTextKind::I32>(ctx, (unsigned)tiles, in, n, vec, counts, tile_base, o_off, o_b); break;
            case NumTextKind::I64: launch_emit<NumTextKind::I64>(ctx, (unsigned)tiles, in, n, vec, counts, tile_base, o_off, o_b); break;
            case NumTextKind::U64: launch_emit<NumTextKind::U64>(ctx, (unsigned)tiles, in, n, vec, counts, tile_base, o_off, o_b); break;
            case NumTextKind::TS: launch_emit<NumTextKind::TS>(ctx, (unsigned)tiles, in, n, vec, counts, tile_base, o_off, o_b); break;
        }
    }
    FG_TRY(check_launch(ctx, "numtext_emit_kernel"));
    out->values = o_b;
    out->bytes = (int64_t)total;
    return FLOCKGPU_OK;
}

}  // namespace flockgpu
