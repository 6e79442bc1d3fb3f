// CAST(x AS Int32 / Int64 / UInt64 / Timestamp(ms)) of a Utf8 column (textnum.hpp A-TN1..A-TN6): one kernel writes the values as a column of the target
// type and their validity bytes, which the expression program (valprog.hpp) then reads as any other column -- the way strlen.hip's lengths reach it.
//   textnum_parse_kernel   utf8_chars_kernel's streaming shape.  A workgroup takes kParseRows consecutive rows and streams the contiguous byte range they
//                          span through LDS in rounds of kParseRoundBytes: every 16 bytes with ONE load at an aligned address, the partial first and
//                          last chunk of that range byte by byte -- no byte outside the rows' range is read.  After the barrier a lane takes rows: the 24
//                          bytes that END where its value ends (integers) or BEGIN where it begins (timestamps) come out of LDS as four ALIGNED 64-bit
//                          words and are lined up with a funnel shift (a misaligned LDS read costs about 6x here: tools/micro/lds_unaligned.hip); what
//                          those words hold outside the value -- a neighbour's bytes, padding -- is masked by the parse (textnum.hpp), which runs in
//                          registers.  Outputs: the value, a validity byte, and for cast_expr ONE failure word per launch in pinned host memory that a
//                          lane stores to only when its value does not parse: no clear, no copy, no wait of its own (the host reads it after the wait
//                          the evaluator has for its own failure word, which a later kernel of the same stream answers).
//                          A value belongs to the round its LAST byte lies in; where it began in the round before, its first bytes are there too: the
//                          lanes that stage a round's last 32 bytes first move what their LDS slots held -- the previous round's last 32 bytes -- into
//                          the padding in front of the round.  A value of more than 24 bytes (a run of leading zeros) takes a PLAIN path before the
//                          rounds: the parse reads its bytes from global memory one at a time.  Correct, not tuned.
//                          A second instance (kRange) parses inside a per-row range [rb[i], re[i]) of the value -- a text slice (textslice.hpp) -- in
//                          place of the offsets; a range that leaves the workgroup's bytes is a value that does not parse, never a read.
#include <algorithm>

#include "gather.hpp"
#include "scan.hpp"
#include "textnum.hpp"
#include "textsel.hpp"

using namespace flockgpu;

namespace {

constexpr int kParseRows = 1024;            // rows of a workgroup
constexpr int kParseRoundBytes = 16384;     // bytes of a round: four 16-byte loads in flight per lane
constexpr int kParseChunks = kParseRoundBytes / 16;
constexpr int kParsePad = 32;               // LDS bytes either side of a round: a window may reach 24 bytes out of it (and 8 more for the aligned read);
                                            // the front ones hold the previous round's last 32 bytes

template <TextNumKind K>
__device__ __forceinline__ void put(void *out, uint8_t *out_valid, int64_t row, uint64_t bits, bool ok) {
    if (K == TextNumKind::I32) static_cast<int32_t *>(out)[row] = ok ? (int32_t)(uint32_t)bits : 0;
    else static_cast<int64_t *>(out)[row] = ok ? (int64_t)bits : 0;
    out_valid[row] = ok ? 1 : 0;
}

template <TextNumKind K, bool kRange>
__global__ __launch_bounds__(kBlock) void textnum_parse_kernel(const int32_t *__restrict__ off, const uint8_t *__restrict__ bytes, const uint8_t *__restrict__ valid, int64_t n_rows,
                                                               const int32_t *__restrict__ rb, const int32_t *__restrict__ re, int32_t try_cast, void *__restrict__ out,
                                                               uint8_t *__restrict__ out_valid, uint32_t *h_fail) {
    __shared__ __attribute__((aligned(16))) uint8_t s_bytes[kParseRoundBytes + 2 * kParsePad];
    __shared__ int32_t s_a[kParseRows], s_b[kParseRows];   // a row's value: bytes [a, b) of the column; b < a: nothing left to do in the rounds
    const int tid = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kParseRows;
    const int32_t nr = (int32_t)(row0 >= n_rows ? 0 : (n_rows - row0 < kParseRows ? n_rows - row0 : kParseRows));
    if (nr <= 0) return;   // (block-uniform)
    const int64_t B0 = off[row0], B1 = off[row0 + nr];
    // u = byte offset + mis: the coordinate in which 16-byte-aligned ADDRESSES are multiples of 16
    const int64_t mis = (int64_t)(reinterpret_cast<uintptr_t>(bytes) & 15u);
    const int64_t base0 = ((B0 + mis) & ~int64_t(15)) - mis;   // byte offset of round 0's position 0 (<= B0)
    bool failed = false;
    for (int r = tid; r < nr; r += kBlock) {
        const int64_t row = row0 + r;
        int32_t a = 0, b = -1;
        if (valid && !valid[row]) {   // NULL in, NULL out
            put<K>(out, out_valid, row, 0, false);
        } else {
            a = kRange ? rb[row] : off[row];
            b = kRange ? re[row] : off[row + 1];
            const int64_t len = (int64_t)b - a;
            if (a < B0 || b > B1 || len <= 0) {   // no byte (or a range outside the workgroup's bytes): not a number
                put<K>(out, out_valid, row, 0, false);
                failed = true;
                b = a - 1;
            } else if (len > kTextNumWindow) {   // the plain path
                uint64_t bits = 0;
                const bool ok = textnum_bytes(K, bytes + a, len, &bits);
                put<K>(out, out_valid, row, bits, ok);
                failed = failed || !ok;
                b = a - 1;
            }
        }
        s_a[r] = a;
        s_b[r] = b;
    }
    const uint64_t *words = reinterpret_cast<const uint64_t *>(s_bytes);
    for (int64_t base = base0; base < B1; base += kParseRoundBytes) {
        uint4 v[kParseChunks / kBlock];
#pragma unroll
        for (int i = 0; i < kParseChunks / kBlock; ++i) {
            const int64_t o = base + (int64_t)(i * kBlock + tid) * 16;
            v[i] = make_uint4(0u, 0u, 0u, 0u);
            if (o >= B0 && o + 16 <= B1) {
                v[i] = stream_load4u(reinterpret_cast<const uint32_t *>(bytes + o));   // (read once: non-temporal)
            } else if (o + 16 > B0 && o < B1) {   // the first / last, partial chunk of the workgroup's bytes: byte by byte, nothing outside them is touched
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                for (int k = 0; k < 16; ++k)
                    if (o + k >= B0 && o + k < B1) w[k >> 2] |= (uint32_t)bytes[o + k] << (8 * (k & 3));
                v[i] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        __syncthreads();   // the previous round's rows are parsed (first round: s_a / s_b are written)
#pragma unroll
        for (int i = 0; i < kParseChunks / kBlock; ++i) {
            const int chunk = i * kBlock + tid;
            uint4 *slot = reinterpret_cast<uint4 *>(s_bytes + kParsePad + chunk * 16);
            // (the round's last two chunks: what the slot held goes in front of the round -- this lane alone touches either place before the barrier;
            // the first round moves bytes nobody looks at)
            if (chunk >= kParseChunks - kParsePad / 16) *reinterpret_cast<uint4 *>(s_bytes + (chunk - (kParseChunks - kParsePad / 16)) * 16) = *slot;
            *slot = v[i];
        }
        __syncthreads();
        for (int r = tid; r < nr; r += kBlock) {
            const int32_t a = s_a[r], b = s_b[r];
            if (b <= a || b <= base || b > base + kParseRoundBytes) continue;   // done, or another round's (a > base - 24: in the padding at worst)
            const int len = b - a;   // [1, 24]
            // the window's first byte in s_bytes: integers end at b, timestamps begin at a
            const int s = (K == TextNumKind::TS ? (int)(a - base) : (int)(b - base) - kTextNumWindow) + kParsePad;   // > 8
            const int q = s >> 3, sh = (s & 7) * 8;
            const uint64_t q0 = words[q], q1 = words[q + 1], q2 = words[q + 2], q3 = words[q + 3];   // (the last: at most byte kParseRoundBytes + 40)
            TextNumWindow x;   // ((hi << 1) << (63 - sh): nothing of hi at sh = 0)
            x.w[0] = (q0 >> sh) | ((q1 << 1) << (63 - sh));
            x.w[1] = (q1 >> sh) | ((q2 << 1) << (63 - sh));
            x.w[2] = (q2 >> sh) | ((q3 << 1) << (63 - sh));
            uint64_t bits = 0;
            bool ok;
            if (K == TextNumKind::TS) {
                int64_t ms = 0;
                ok = textnum_ts(x, len, &ms);
                bits = (uint64_t)ms;
            } else {
                ok = textnum_int(K, x, len, &bits);
            }
            put<K>(out, out_valid, row0 + r, bits, ok);
            failed = failed || !ok;
        }
    }
    if (failed && !try_cast) __atomic_store_n(h_fail, 1u, __ATOMIC_RELAXED);   // (pinned host memory; every failing lane stores the same word)
}

template <TextNumKind K>
void launch_parse(flockgpu_ctx *ctx, unsigned grid, const DevColumn &col, int64_t rows, const int32_t *rb, const int32_t *re, bool try_cast, void *out, uint8_t *out_valid, uint32_t *h_fail) {
    const uint8_t *bytes = static_cast<const uint8_t *>(col.values);
    if (rb) hipLaunchKernelGGL((textnum_parse_kernel<K, true>), dim3(grid), dim3(kBlock), 0, ctx->stream, col.offsets, bytes, col.valid, rows, rb, re, (int32_t)try_cast, out, out_valid, h_fail);
    else hipLaunchKernelGGL((textnum_parse_kernel<K, false>), dim3(grid), dim3(kBlock), 0, ctx->stream, col.offsets, bytes, col.valid, rows, nullptr, nullptr, (int32_t)try_cast, out, out_valid, h_fail);
}

}  // namespace

namespace flockgpu {

int text_to_num(flockgpu_ctx *ctx, const char *name, const DevColumn &col, int64_t rows, TextNumKind kind, bool try_cast, const int32_t *range_begin, const int32_t *range_end,
                DevColumn *out, const uint32_t **h_fail) {
    const std::string base = name;
    *out = DevColumn{};
    out->type = kind == TextNumKind::I32 ? ColType::I32 : kind == TextNumKind::U64 ? ColType::U64 : ColType::I64;
    out->is_ts = kind == TextNumKind::TS;
    out->nullable = true;
    *h_fail = nullptr;
    if (col.type != ColType::UTF8 || !col.offsets) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: not a Utf8 column", name);
    if ((range_begin == nullptr) != (range_end == nullptr)) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: a range takes both arrays", name);
    if (rows >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than 2^31 rows", name);
    const int64_t n = std::max<int64_t>(rows, 0);
    void *vals = nullptr;
    uint8_t *vv = nullptr;
    uint32_t *flag = nullptr;
    FG_TRY(arena_get(ctx, (base + ".val").c_str(), ((size_t)n + 2) * 8, &vals));
    FG_TRY(arena_get_t(ctx, (base + ".valid").c_str(), (size_t)n + 16, &vv));
    FG_TRY(pinned_get_t(ctx, (base + ".fail").c_str(), 4, &flag));
    out->values = vals;
    out->valid = vv;
    __atomic_store_n(flag, 0u, __ATOMIC_RELAXED);   // (no kernel that writes it is in flight: the execute that queued one has waited behind it)
    *h_fail = flag;
    if (n == 0) return FLOCKGPU_OK;
    const unsigned grid = (unsigned)div_up(n, kParseRows);
    {
        LaunchScope ls(ctx, "textnum_parse_kernel");
        switch (kind) {
            case TextNumKind::I32: launch_parse<TextNumKind::I32>(ctx, grid, col, n, range_begin, range_end, try_cast, vals, vv, flag); break;
            case TextNumKind::I64: launch_parse<TextNumKind::I64>(ctx, grid, col, n, range_begin, range_end, try_cast, vals, vv, flag); break;
            case TextNumKind::U64: launch_parse<TextNumKind::U64>(ctx, grid, col, n, range_begin, range_end, try_cast, vals, vv, flag); break;
            case TextNumKind::TS: launch_parse<TextNumKind::TS>(ctx, grid, col, n, range_begin, range_end, try_cast, vals, vv, flag); break;
        }
    }
    return check_launch(ctx, "textnum_parse_kernel");
}

}  // namespace flockgpu
