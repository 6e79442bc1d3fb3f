// octet_length / char_length of a Utf8 column (valprog.hpp A-F7): one kernel per (column, function) writes the lengths as an Int32 column, which the
// expression program then reads as any other column.
//   utf8_octets_kernel   offsets only: off[i + 1] - off[i].
//   utf8_chars_kernel    code points = bytes that are not 10xxxxxx.  A workgroup takes 2048 consecutive rows and streams the contiguous byte range they
//                        span in rounds of kLenRoundBytes, every 16 bytes with ONE load at an aligned address (the partial first and last chunk of
//                        that range byte by byte, as strmatch_contains_kernel does at the buffer's ends: no byte outside the rows is read).  A lane reduces its chunk in registers to a 16-bit mask of the bytes
//                        that begin a code point and stages the MASK in LDS -- a sixteenth of the bytes; nothing else of them is needed.  After the
//                        barrier a lane takes rows: it counts the bits of the mask words its row covers in this round (64 positions per word) and adds
//                        them to the row's count in LDS.  A row that straddles rounds collects its count over them; a row longer than a round is
//                        just more words.  Global loads: the offsets and the chunks, none under a per-row branch.
//                        A second instance (kRange) counts inside a per-row range [rb[i], re[i]) of the value -- an inner text slice
//                        (textslice.hpp) -- instead of the whole value; the plain instance's code is what it was.
#include <algorithm>

#include "gather.hpp"
#include "scan.hpp"
#include "valprog.hpp"

using namespace flockgpu;

namespace {

constexpr int kLenRows = 2048;              // rows of a workgroup
constexpr int kLenRoundBytes = 32768;       // bytes of a round: eight 16-byte loads in flight per lane
constexpr int kLenChunks = kLenRoundBytes / 16;

__global__ __launch_bounds__(kBlock) void utf8_octets_kernel(const int32_t *__restrict__ off, int64_t n_rows, int32_t *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_rows; i += (int64_t)gridDim.x * kBlock) out[i] = off[i + 1] - off[i];
}

// bit k: byte k of the chunk is not a continuation byte
__device__ __forceinline__ uint32_t lead_mask4(uint32_t w) {
    const uint32_t cont = w & (~w << 1) & 0x80808080u;   // bit 7 of a byte: 1 where the byte is 10xxxxxx
    const uint32_t lead = ~cont & 0x80808080u;
    return ((lead >> 7) & 1u) | ((lead >> 14) & 2u) | ((lead >> 21) & 4u) | ((lead >> 28) & 8u);
}

template <bool kRange>
__global__ __launch_bounds__(kBlock) void utf8_chars_kernel(const int32_t *__restrict__ off, const uint8_t *__restrict__ bytes, int64_t n_rows,
                                                            const int32_t *__restrict__ rb, const int32_t *__restrict__ re, int32_t *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint16_t s_mask[kLenChunks + 4];   // (+ 4: the last word read whole)
    __shared__ int32_t s_off[kLenRows + 1];
    __shared__ int32_t s_cnt[kLenRows];
    __shared__ int32_t s_rb[kRange ? kLenRows : 1], s_re[kRange ? kLenRows : 1];   // kRange: the rows' ranges
    const int tid = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kLenRows;
    const int32_t nr = (int32_t)(row0 >= n_rows ? 0 : (n_rows - row0 < kLenRows ? n_rows - row0 : kLenRows));
    if (nr <= 0) return;   // (block-uniform)
    for (int i = tid; i <= nr; i += kBlock) s_off[i] = off[row0 + i];
    for (int i = tid; i < nr; i += kBlock) s_cnt[i] = 0;
    if (kRange)
        for (int i = tid; i < nr; i += kBlock) {
            s_rb[i] = rb[row0 + i];
            s_re[i] = re[row0 + i];
        }
    if (tid < 4) s_mask[kLenChunks + tid] = 0;
    __syncthreads();
    const int64_t B0 = s_off[0], B1 = s_off[nr];
    const uint64_t *mask64 = reinterpret_cast<const uint64_t *>(s_mask);
    // u = byte offset + mis: the coordinate in which 16-byte-aligned ADDRESSES are multiples of 16
    const int64_t mis = (int64_t)(reinterpret_cast<uintptr_t>(bytes) & 15u);
    for (int64_t G = (B0 + mis) & ~int64_t(15); G - mis < B1; G += kLenRoundBytes) {
        const int64_t base = G - mis;   // byte offset of the round's position 0
        uint32_t m[kLenChunks / kBlock];
#pragma unroll
        for (int i = 0; i < kLenChunks / kBlock; ++i) {
            const int64_t o = base + (int64_t)(i * kBlock + tid) * 16;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (o >= B0 && o + 16 <= B1) {
                v = stream_load4u(reinterpret_cast<const uint32_t *>(bytes + o));   // (read once: non-temporal)
            } else if (o + 16 > B0 && o < B1) {   // the first / last, partial chunk of the workgroup's bytes: byte by byte, nothing outside them is touched
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                for (int k = 0; k < 16; ++k)
                    if (o + k >= B0 && o + k < B1) w[k >> 2] |= (uint32_t)bytes[o + k] << (8 * (k & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            m[i] = lead_mask4(v.x) | (lead_mask4(v.y) << 4) | (lead_mask4(v.z) << 8) | (lead_mask4(v.w) << 12);
        }
        __syncthreads();   // the previous round's counts are taken
#pragma unroll
        for (int i = 0; i < kLenChunks / kBlock; ++i) s_mask[i * kBlock + tid] = (uint16_t)m[i];
        __syncthreads();
        for (int r = tid; r < nr; r += kBlock) {
            int64_t a = (int64_t)(kRange ? s_rb[r] : s_off[r]) - base, b = (int64_t)(kRange ? s_re[r] : s_off[r + 1]) - base;   // the row's positions in this round: [a, b)
            a = a < 0 ? 0 : a;
            b = b > kLenRoundBytes ? kLenRoundBytes : b;
            if (a >= b) continue;
            int32_t c = 0;
            for (int w = (int)(a >> 6); w <= (int)((b - 1) >> 6); ++w) {
                uint64_t x = mask64[w];
                const int64_t lo = (int64_t)w << 6;
                if (a > lo) x &= ~uint64_t(0) << (a - lo);
                if (b < lo + 64) x &= ~uint64_t(0) >> (lo + 64 - b);
                c += __popcll(x);
            }
            s_cnt[r] += c;
        }
    }
    __syncthreads();
    for (int i = tid; i < nr; i += kBlock) out[row0 + i] = s_cnt[i];
}

}  // namespace

namespace flockgpu {

int utf8_lengths(flockgpu_ctx *ctx, const char *name, const DevColumn &col, int64_t rows, bool code_points, int32_t **out, const int32_t *range_begin,
                 const int32_t *range_end) {
    int32_t *len = nullptr;
    FG_TRY(arena_get_t(ctx, name, (size_t)std::max<int64_t>(rows, 0) + 4, &len));
    *out = len;
    if (rows <= 0) return FLOCKGPU_OK;
    if (rows >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than 2^31 rows", name);
    if (col.type != ColType::UTF8 || !col.offsets) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: not a Utf8 column", name);
    if ((range_begin == nullptr) != (range_end == nullptr) || (range_begin && !code_points)) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: a range takes both arrays and counts code points", name);
    if (!code_points) {
        const unsigned grid = (unsigned)std::min<int64_t>(div_up(rows, kBlock), (int64_t)ctx->num_cus * 16);
        LaunchScope ls(ctx, "utf8_octets_kernel");
        hipLaunchKernelGGL(utf8_octets_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, col.offsets, rows, len);
        return check_launch(ctx, "utf8_octets_kernel");
    }
    LaunchScope ls(ctx, "utf8_chars_kernel");
    const dim3 grid((unsigned)div_up(rows, kLenRows));
    const uint8_t *bytes = static_cast<const uint8_t *>(col.values);
    if (range_begin) hipLaunchKernelGGL(utf8_chars_kernel<true>, grid, dim3(kBlock), 0, ctx->stream, col.offsets, bytes, rows, range_begin, range_end, len);
    else hipLaunchKernelGGL(utf8_chars_kernel<false>, grid, dim3(kBlock), 0, ctx->stream, col.offsets, bytes, rows, nullptr, nullptr, len);
    return check_launch(ctx, "utf8_chars_kernel");
}

}  // namespace flockgpu
