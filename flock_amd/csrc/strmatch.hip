// Utf8 LIKE and ordered comparisons against a literal (strmatch.hpp): one kernel per (column, pattern) leaf writes the leaf's TRUE bits as flag-tile
// words, which the predicate program reads through a Words leaf.
//   strmatch_contains_kernel  `%needle%` (one piece, no `_`): byte-parallel.  A workgroup streams the contiguous byte range of its rows through an
//                             LDS stage in rounds of kStrStageBytes; lanes test byte POSITIONS with windows shifted in registers, and a hit finds its
//                             row by a binary search in the rows' offsets (LDS) and sets the row's bit by an LDS atomic OR.
//   strmatch_rows_kernel      every other pattern, and the ordered comparisons: the greedy matcher, row per lane slot in the flag-tile geometry.  An
//                             anchored pattern (`lit`, `lit%`, `%lit`, `a%b`) touches only the first / last pattern-length bytes of a value here, too.
#include <algorithm>
#include <cstring>

#include "gather.hpp"
#include "scan.hpp"
#include "strmatch.hpp"

using namespace flockgpu;

namespace {

__device__ __forceinline__ bool is_cont(uint8_t b) { return (b & 0xC0u) == 0x80u; }

// piece [a, b) of the pattern forwards from byte p of the value that ends at `end`; *q: the byte after the match
__device__ __forceinline__ bool piece_fwd(const StrPattern &P, int a, int b, const uint8_t *__restrict__ v, int32_t p, int32_t end, int32_t *q_out) {
    int32_t q = p;
    for (int k = a; k < b; ++k) {   // (uniform trip count)
        const uint8_t c = P.bytes[k];
        if (q >= end) return false;
        const uint8_t x = v[q];
        if (c == '_') {
            if (is_cont(x)) return false;
            ++q;
            while (q < end && is_cont(v[q])) ++q;
        } else {
            if (x != c) return false;
            ++q;
        }
    }
    *q_out = q;
    return true;
}
// ... backwards from the value's end `e`, never below `lo`; *q: the first byte of the match
__device__ __forceinline__ bool piece_bwd(const StrPattern &P, int a, int b, const uint8_t *__restrict__ v, int32_t lo, int32_t e, int32_t *q_out) {
    int32_t q = e;
    for (int k = b - 1; k >= a; --k) {
        const uint8_t c = P.bytes[k];
        if (q <= lo) return false;
        --q;
        if (c == '_') {
            while (q > lo && is_cont(v[q])) --q;
            if (is_cont(v[q])) return false;
        } else if (v[q] != c) {
            return false;
        }
    }
    *q_out = q;
    return true;
}

__device__ __forceinline__ bool like_row(const StrPattern &P, const uint8_t *__restrict__ v, int32_t b0, int32_t b1) {
    const int n = P.n_pieces;
    int32_t pos = b0;
    if (!piece_fwd(P, P.piece_off[0], P.piece_off[1], v, b0, b1, &pos)) return false;
    if (n == 1) return pos == b1;
    int32_t limit = b1;
    if (!piece_bwd(P, P.piece_off[n - 1], P.piece_off[n], v, pos, b1, &limit)) return false;
    for (int m = 1; m + 1 < n; ++m) {
        const int a = P.piece_off[m], b = P.piece_off[m + 1];
        bool found = false;
        for (int32_t p = pos; p <= limit - (b - a) && !found; ++p) {   // (a piece is at least as many bytes as it has elements)
            int32_t q;
            if (piece_fwd(P, a, b, v, p, limit, &q)) {
                pos = q;
                found = true;
            }
        }
        if (!found) return false;
    }
    return true;
}

__device__ __forceinline__ bool cmp_row(const StrPattern &P, const uint8_t *__restrict__ v, int32_t b0, int32_t b1) {
    const int32_t la = b1 - b0, n = la < P.len ? la : P.len;
    int32_t k = 0;
    while (k < n && v[b0 + k] == P.bytes[k]) ++k;
    bool lt, eq = false;
    if (k < n) {
        lt = v[b0 + k] < P.bytes[k];
    } else {
        lt = la < P.len;
        eq = la == P.len;
    }
    switch (P.op) {   // (uniform)
        case (uint8_t)StrOp::Lt: return lt;
        case (uint8_t)StrOp::Le: return lt || eq;
        case (uint8_t)StrOp::Gt: return !lt && !eq;
        default: return !lt;
    }
}

// grid (tiles) -- or, kSplit, (tiles, 8): workgroup (t, s) takes iteration s of tile t only and ORs its four bits per lane into the words the host
// cleared (a relation of a few tiles: a row's match is a chain of dependent loads, as pred.hip's leaves are).  Every load is guarded by the row count.
template <bool kSplit>
__global__ __launch_bounds__(kBlock) void strmatch_rows_kernel(const StrPattern P, const int32_t *__restrict__ off, const uint8_t *__restrict__ bytes, int64_t n_rows,
                                                               uint32_t *__restrict__ words) {
    const int64_t wbase = (int64_t)blockIdx.x * kFlagTile + flag_rel0();
    uint32_t bits = 0;
#pragma unroll 1
    for (int it = 0; it < kFlagIters; ++it) {
        if (kSplit && it != (int)blockIdx.y) continue;
        const int64_t r0 = wbase + it * 256;
        int32_t o[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int64_t r = r0 + j > n_rows ? n_rows : r0 + j;
            o[j] = off[r];
        }
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            if (r0 + j >= n_rows) break;
            const int32_t b0 = j == 0 ? o[0] : j == 1 ? o[1] : j == 2 ? o[2] : o[3];
            const int32_t b1 = j == 0 ? o[1] : j == 1 ? o[2] : j == 2 ? o[3] : o[4];
            const bool hit = P.op == (uint8_t)StrOp::Like ? like_row(P, bytes, b0, b1) : cmp_row(P, bytes, b0, b1);
            bits |= (uint32_t)hit << (it * 4 + j);
        }
    }
    uint32_t *w = words + (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (kSplit) {
        if (bits) atomicOr(w, bits);
    } else {
        *w = bits;
    }
}

// ---- `%needle%`
constexpr int kStageKeep = kStrMaxPattern;                          // bytes of the previous round kept in front of a round's own (>= needle - 1)
constexpr int kStageChunks = (kStageKeep + kStrStageBytes) / 16;   // 16-byte chunks a round tests

// grid (tiles, 4): workgroup (t, w) takes the 2048 consecutive rows whose flags are wave w's 64 words of tile t, and stores those words itself (nothing to
// clear, no atomics on global memory).  2048 offsets + the stage are 25 KB of LDS: six workgroups per CU.
__global__ __launch_bounds__(kBlock) void strmatch_contains_kernel(const StrPattern P, const int32_t *__restrict__ off, const uint8_t *__restrict__ bytes, int64_t total,
                                                                   int64_t n_rows, uint32_t *__restrict__ words) {
    constexpr int32_t rows_per_block = kFlagWaveRows;
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[kStageKeep + kStrStageBytes + 16];
    __shared__ int32_t s_off[kFlagWaveRows + 1];
    __shared__ uint32_t s_bits[64];
    const int tid = (int)threadIdx.x;
    const int64_t tile_row0 = (int64_t)blockIdx.x * kFlagTile;
    const int32_t rel_first = (int32_t)blockIdx.y * rows_per_block;
    const int64_t row0 = tile_row0 + rel_first;   // (rel_first: the wave's first row in the tile)
    const int32_t nr = (int32_t)(row0 >= n_rows ? 0 : (n_rows - row0 < rows_per_block ? n_rows - row0 : rows_per_block));
    if (tid < 64) s_bits[tid] = 0;
    for (int i = tid; i <= nr && nr > 0; i += kBlock) s_off[i] = off[row0 + i];
    uint4 *stage4 = reinterpret_cast<uint4 *>(s_stage);
    if (tid == 0) stage4[kStageChunks] = make_uint4(0u, 0u, 0u, 0u);   // (the last chunk's windows look four bytes past the round)
    __syncthreads();
    if (nr > 0) {
        const int32_t B0 = s_off[0], B1 = s_off[nr];
        const int L = P.len;
        uint32_t first4 = 0;
        for (int k = 0; k < 4 && k < L; ++k) first4 |= (uint32_t)P.bytes[k] << (8 * k);
        const uint32_t mask4 = L >= 4 ? ~0u : ((1u << (8 * L)) - 1u);
        // u = byte offset + mis: the coordinate in which 16-byte-aligned ADDRESSES are multiples of 16
        const int64_t mis = (int64_t)(reinterpret_cast<uintptr_t>(bytes) & 15u);
        int round = 0;
        for (int64_t G = ((int64_t)B0 + mis) & ~int64_t(15); G - mis < B1; G += kStrStageBytes, ++round) {
            uint4 tail = make_uint4(0u, 0u, 0u, 0u);
            if (tid < kStageKeep / 16 && round > 0) tail = stage4[kStrStageBytes / 16 + tid];
            __syncthreads();   // the previous round's tests are done
            if (tid < kStageKeep / 16) stage4[tid] = tail;
#pragma unroll
            for (int i = 0; i < kStrStageBytes / 16 / kBlock; ++i) {
                const int c = i * kBlock + tid;
                const int64_t o = G - mis + (int64_t)c * 16;   // byte offset of the chunk
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (o >= 0 && o + 16 <= total) {
                    v = stream_load4u(reinterpret_cast<const uint32_t *>(bytes + o));   // (read once: non-temporal)
                } else if (o + 16 > 0 && o < total) {   // the buffer's first / last, partial chunk: byte by byte
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
                    for (int k = 0; k < 16; ++k)
                        if (o + k >= 0 && o + k < total) w[k >> 2] |= (uint32_t)bytes[o + k] << (8 * (k & 3));
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                }
                stage4[kStageKeep / 16 + c] = v;
            }
            __syncthreads();
            const int64_t base = G - mis - kStageKeep;   // byte offset of stage position 0
            for (int c = tid; c < kStageChunks; c += kBlock) {
                const uint4 a = stage4[c];
                const uint32_t w[5] = {a.x, a.y, a.z, a.w, *reinterpret_cast<const uint32_t *>(s_stage + (c + 1) * 16)};
                uint32_t hits = 0;
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const int i = s >> 2, sh = (s & 3) * 8;
                    const uint32_t win = sh ? (w[i] >> sh) | (w[i + 1] << (32 - sh)) : w[i];
                    hits |= (uint32_t)(((win ^ first4) & mask4) == 0u) << s;
                }
                while (hits) {   // rare for any needle worth writing
                    const int s = __ffs((int)hits) - 1;
                    hits &= hits - 1u;
                    const int p = c * 16 + s;
                    const int64_t o = base + p;
                    if (o < B0 || o + L > B1 || p + L > kStageKeep + kStrStageBytes) continue;   // (past the stage: the next round sees it whole)
                    bool same = true;
                    for (int k = 4; k < L && same; ++k) same = s_stage[p + k] == P.bytes[k];
                    if (!same) continue;
                    int lo = 0, hi = nr;   // the row that holds byte o: the largest i with s_off[i] <= o
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if ((int64_t)s_off[mid] <= o) lo = mid; else hi = mid;
                    }
                    if (o + L > (int64_t)s_off[lo + 1]) continue;   // the needle lies across two rows: no match
                    atomicOr(&s_bits[(lo & 255) >> 2], 1u << ((lo >> 8) * 4 + (lo & 3)));   // row lo of the wave's 2048: lane (lo % 256) / 4, bit (lo / 256) * 4 + lo % 4
                }
            }
        }
    }
    __syncthreads();
    if (tid < 64) words[(size_t)blockIdx.x * kBlock + blockIdx.y * 64 + tid] = s_bits[tid];
}

}  // namespace

namespace flockgpu {

bool strmatch_compile_like(const std::string &pattern, StrPattern *out, std::string *why) {
    StrPattern p{};
    p.op = (uint8_t)StrOp::Like;
    int pieces = 1;
    for (char ch : pattern) {
        if (ch == '%') {
            if (pieces >= kStrMaxPieces) { *why = "more than " + std::to_string(kStrMaxPieces - 1) + " '%' in the pattern"; return false; }
            p.piece_off[pieces++] = (uint8_t)p.len;
            continue;
        }
        if (p.len >= kStrMaxPattern) { *why = "a pattern of more than " + std::to_string(kStrMaxPattern) + " bytes"; return false; }
        if (ch == '_') p.has_underscore = 1;
        p.bytes[p.len++] = (uint8_t)ch;
    }
    p.piece_off[pieces] = (uint8_t)p.len;
    p.n_pieces = pieces;
    *out = p;
    return true;
}

bool strmatch_compile_cmp(const std::string &literal, int cmp_op, StrPattern *out, std::string *why) {
    StrPattern p{};
    if (literal.size() > (size_t)kStrMaxPattern) { *why = "a literal of more than " + std::to_string(kStrMaxPattern) + " bytes"; return false; }
    p.op = (uint8_t)cmp_op;
    p.len = (int32_t)literal.size();
    std::memcpy(p.bytes, literal.data(), literal.size());
    p.n_pieces = 1;
    p.piece_off[1] = (uint8_t)p.len;
    *out = p;
    return true;
}

int strmatch_words(flockgpu_ctx *ctx, const char *name, const DevColumn &col, int64_t rows, const StrPattern &pat, uint32_t **out_words) {
    const int64_t n_tiles = std::max<int64_t>(div_up(std::max<int64_t>(rows, 0), kFlagTile), 0);
    uint32_t *words = nullptr;
    FG_TRY(arena_get_t(ctx, name, (size_t)n_tiles * kBlock + 4, &words));
    *out_words = words;
    if (rows <= 0) return FLOCKGPU_OK;
    if (rows >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than 2^31 rows", name);
    const int32_t *off = col.offsets;
    const uint8_t *bytes = static_cast<const uint8_t *>(col.values);
    // `%needle%`: three pieces, the outer two empty, no `_`
    const bool contains = pat.op == (uint8_t)StrOp::Like && pat.n_pieces == 3 && pat.piece_off[1] == 0 && pat.piece_off[2] == pat.len && pat.len > 0 && !pat.has_underscore;
    if (contains) {
        LaunchScope ls(ctx, "strmatch_contains_kernel");
        hipLaunchKernelGGL(strmatch_contains_kernel, dim3((unsigned)n_tiles, kWavesPerBlock), dim3(kBlock), 0, ctx->stream, pat, off, bytes, col.bytes, rows, words);
        return check_launch(ctx, "strmatch_contains_kernel");
    }
    const bool few = n_tiles < 4 * (int64_t)ctx->num_cus;
    if (few) FG_TRY(fill_words(ctx, FillList().add(words, 0u, (uint64_t)n_tiles * kBlock)));
    LaunchScope ls(ctx, "strmatch_rows_kernel");
    if (few) hipLaunchKernelGGL((strmatch_rows_kernel<true>), dim3((unsigned)n_tiles, kFlagIters), dim3(kBlock), 0, ctx->stream, pat, off, bytes, rows, words);
    else hipLaunchKernelGGL((strmatch_rows_kernel<false>), dim3((unsigned)n_tiles), dim3(kBlock), 0, ctx->stream, pat, off, bytes, rows, words);
    return check_launch(ctx, "strmatch_rows_kernel");
}

}  // namespace flockgpu
