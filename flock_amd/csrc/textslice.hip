// Text slice functions (textslice.hpp): per row the (begin, end) byte positions of split_part / left / right / ltrim / rtrim / btrim.
//   text_slice_stream_kernel   the bytewise classes (a one-byte delimiter, lead bytes, an ASCII trim set): utf8_chars_kernel's streaming shape
//                              (strlen.hip) with the class mask in LDS and, per row, the k-th / last set bit of the mask inside the row's range.
//                              Global loads: the offsets (or the inner call's pairs), the per-row counts where k is per row, and the chunks -- all
//                              before the rounds or as the round's aligned 16-byte loads, none under a per-row branch.  LDS is read as aligned
//                              64-bit mask words and aligned 32-bit row state.
//   text_slice_general_kernel  a delimiter of 2 to 16 bytes, a trim set with a non-ASCII code point: one lane per row walks its value.
// Every row index is checked against the row count; the row pass reads LDS only, at positions clipped to the round, so whatever a NULL row's offsets
// (or an inner call's pair) hold cannot take a read outside the masks.
#include <algorithm>

#include "gather.hpp"
#include "scan.hpp"
#include "textslice.hpp"
#include "textslice_bits.hpp"
#include "valprog.hpp"

using namespace flockgpu;
using namespace flockgpu::slicebits;

namespace {

constexpr int kSliceChunks = kSliceRoundBytes / 16;
constexpr uint32_t kAtStart = 0xffffffffu;   // a target that is never found and whose default is the row's START
constexpr uint32_t kNever = 0x80000000u;     // a target beyond any count (a column holds fewer than 2^31 bytes)
static_assert(kSliceChunks % kBlock == 0, "a round is a whole number of chunks per lane");
static_assert(kSliceRows % kBlock == 0, "rows per lane");

// What the streaming kernel selects (textslice.hpp): a target is the 1-based index of a set bit inside the row's range.
struct StreamParams {
    uint32_t kb;       // begin = the position of set bit kb (+ adj); 0: the row's start; not found: the row's end
    uint32_t ke;       // end = the position of set bit ke; 0 or not found: the row's end; kAtStart: the row's start
    uint32_t adj;      // split_part: begin lies one past the delimiter
    uint32_t last;     // 1: end = one past the LAST set bit (none: end = begin)
    int32_t row_to;    // the per-row k replaces 0: nothing, 1: kb, 2: ke -- k = krow[i] - row_sub; k <= 0: the row's start, else target k + 1
    int64_t row_sub;
    uint32_t delim;    // kEqual: the byte
    AsciiSet set;      // kOutside: the characters
};

template <int kClass>
__global__ __launch_bounds__(kBlock) void text_slice_stream_kernel(const int32_t *__restrict__ off, const uint8_t *__restrict__ bytes, int64_t n_rows,
                                                                   const int32_t *__restrict__ in_begin, const int32_t *__restrict__ in_end,
                                                                   const int32_t *__restrict__ krow, StreamParams P, int32_t *__restrict__ out_begin,
                                                                   int32_t *__restrict__ out_end) {
    __shared__ __attribute__((aligned(16))) uint16_t s_mask[kSliceChunks + 4];   // (+ 4: the last word read whole)
    __shared__ int32_t s_a[kSliceRows], s_b[kSliceRows];          // the row's range [a, b): absolute byte positions
    __shared__ uint32_t s_tb[kSliceRows], s_te[kSliceRows];       // the row's targets
    __shared__ uint32_t s_cnt[kSliceRows];                        // set bits of the row seen in earlier rounds
    __shared__ int32_t s_begin[kSliceRows], s_end[kSliceRows];    // the result so far (s_end < 0 with P.last: no set bit yet)
    const int tid = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kSliceRows;
    const int32_t nr = (int32_t)(row0 >= n_rows ? 0 : (n_rows - row0 < kSliceRows ? n_rows - row0 : kSliceRows));
    if (nr <= 0) return;   // (block-uniform)
    for (int i = tid; i < nr; i += kBlock) {
        const int32_t a = in_begin ? in_begin[row0 + i] : off[row0 + i], b = in_end ? in_end[row0 + i] : off[row0 + i + 1];
        uint32_t tb = P.kb, te = P.ke;
        if (P.row_to) {
            const int64_t k = (int64_t)krow[row0 + i] - P.row_sub;
            const uint32_t t = k <= 0 ? (P.row_to == 1 ? 0u : kAtStart) : (uint32_t)(k + 1);
            if (P.row_to == 1) tb = t;
            else te = t;
        }
        s_a[i] = a;
        s_b[i] = b;
        s_tb[i] = tb;
        s_te[i] = te;
        s_cnt[i] = 0;
        s_begin[i] = tb == 0 ? a : b;
        s_end[i] = P.last ? -1 : (te == kAtStart ? a : b);
    }
    if (tid < 4) s_mask[kSliceChunks + tid] = 0;
    // the bytes the workgroup's rows span (the column's own offsets: an inner call's pairs lie inside them)
    const int64_t B0 = off[row0], B1 = off[row0 + nr];
    __syncthreads();
    const uint64_t *mask64 = reinterpret_cast<const uint64_t *>(s_mask);
    // u = byte offset + mis: the coordinate in which 16-byte-aligned ADDRESSES are multiples of 16
    const int64_t mis = (int64_t)(reinterpret_cast<uintptr_t>(bytes) & 15u);
    for (int64_t G = (B0 + mis) & ~int64_t(15); G - mis < B1; G += kSliceRoundBytes) {
        const int64_t base = G - mis;   // byte offset of the round's position 0
        uint32_t m[kSliceChunks / kBlock];
#pragma unroll
        for (int i = 0; i < kSliceChunks / kBlock; ++i) {
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
            // (a chunk or byte outside the workgroup's bytes is zero here; every row clips the mask to its own range)
            m[i] = chunk_mask<kClass>(v.x, v.y, v.z, v.w, (uint8_t)P.delim, P.set);
        }
        __syncthreads();   // the previous round's masks are read
#pragma unroll
        for (int i = 0; i < kSliceChunks / kBlock; ++i) s_mask[i * kBlock + tid] = (uint16_t)m[i];
        __syncthreads();
        for (int r = tid; r < nr; r += kBlock) {
            int64_t a = (int64_t)s_a[r] - base, b = (int64_t)s_b[r] - base;   // the row's positions in this round: [a, b)
            a = a < 0 ? 0 : a;
            b = b > kSliceRoundBytes ? kSliceRoundBytes : b;
            if (a >= b) continue;
            uint32_t c = s_cnt[r];
            const uint32_t tb = s_tb[r], te = s_te[r];
            // nothing left to find: a target is found once the count has reached it, and 0 / kAtStart never are
            if (!P.last && (tb == 0 || tb - 1u < c) && (te == 0 || te == kAtStart || te - 1u < c)) continue;
            int32_t ob = s_begin[r], oe = s_end[r];
            for (int w = (int)(a >> 6); w <= (int)((b - 1) >> 6); ++w) {
                const int64_t lo = (int64_t)w << 6;
                const uint64_t x = clip_word(mask64[w], lo, a, b);
                const uint32_t p = (uint32_t)popcount64(x);
                if (tb - c - 1u < p) ob = (int32_t)(base + lo + select64(x, (int)(tb - c - 1u)) + P.adj);
                if (te - c - 1u < p) oe = (int32_t)(base + lo + select64(x, (int)(te - c - 1u)));
                if (P.last && x) oe = (int32_t)(base + lo + highest64(x) + 1);
                c += p;
            }
            s_cnt[r] = c;
            s_begin[r] = ob;
            s_end[r] = oe;
        }
    }
    __syncthreads();
    for (int i = tid; i < nr; i += kBlock) {
        const int32_t ob = s_begin[i], oe = s_end[i];
        out_begin[row0 + i] = ob;
        out_end[row0 + i] = oe < 0 ? ob : oe;
    }
}

struct GeneralParams {
    int32_t fn;      // SliceFn
    int32_t n;       // split_part: the field
    uint32_t len;    // split_part: bytes of the delimiter; the trims: code points of the set
    uint32_t v[16];  // split_part: the delimiter's bytes, four per word; the trims: a code point's bytes each, the first lowest
};

// the code point that begins at byte i of [.., e): its bytes packed like GeneralParams::v (0xffffffff: longer than four bytes), *len = its bytes
__device__ __forceinline__ uint32_t code_point_at(const uint8_t *__restrict__ bytes, int64_t i, int64_t e, int *len) {
    int l = 1;
    while (i + l < e && (bytes[i + l] & 0xc0u) == 0x80u) ++l;
    *len = l;
    if (l > 4) return 0xffffffffu;
    uint32_t v = 0;
    for (int k = 0; k < l; ++k) v |= (uint32_t)bytes[i + k] << (8 * k);
    return v;
}

__global__ __launch_bounds__(kBlock) void text_slice_general_kernel(const int32_t *__restrict__ off, const uint8_t *__restrict__ bytes, int64_t n_rows,
                                                                    const int32_t *__restrict__ in_begin, const int32_t *__restrict__ in_end, GeneralParams P,
                                                                    int32_t *__restrict__ out_begin, int32_t *__restrict__ out_end) {
    __shared__ uint32_t s_v[16];
    if (threadIdx.x < 16) s_v[threadIdx.x] = P.v[threadIdx.x];
    __syncthreads();
    const uint8_t *s_delim = reinterpret_cast<const uint8_t *>(s_v);
    auto in_set = [&](uint32_t cp) {
        bool hit = false;
        for (uint32_t k = 0; k < P.len; ++k) hit = hit || s_v[k] == cp;
        return hit;
    };
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * kBlock) {
        const int64_t a = in_begin ? in_begin[r] : off[r], b = in_end ? in_end[r] : off[r + 1];
        int64_t ob = a, oe = b;
        if (P.fn == (int32_t)SliceFn::SplitPart) {   // greedy, leftmost, non-overlapping
            const int64_t dl = P.len;
            int64_t i = a, start = a;
            int32_t field = 1;
            bool found = false;
            while (i + dl <= b) {
                bool match = true;
                for (int64_t k = 0; k < dl && match; ++k) match = bytes[i + k] == s_delim[k];
                if (!match) { ++i; continue; }
                if (field == P.n) { ob = start; oe = i; found = true; break; }
                ++field;
                i += dl;
                start = i;
            }
            if (!found) {
                ob = field == P.n ? start : b;
                oe = b;
            }
        } else {
            if (P.fn == (int32_t)SliceFn::Ltrim || P.fn == (int32_t)SliceFn::Btrim)
                while (ob < oe) {
                    int l = 1;
                    if (!in_set(code_point_at(bytes, ob, oe, &l))) break;
                    ob += l;
                }
            if (P.fn == (int32_t)SliceFn::Rtrim || P.fn == (int32_t)SliceFn::Btrim)
                while (oe > ob) {
                    int64_t p = oe - 1;
                    while (p > ob && (bytes[p] & 0xc0u) == 0x80u) --p;
                    int l = 1;
                    if (!in_set(code_point_at(bytes, p, oe, &l))) break;
                    oe = p;
                }
        }
        out_begin[r] = (int32_t)ob;
        out_end[r] = (int32_t)oe;
    }
}

bool all_ascii(const std::string &s) {
    for (unsigned char ch : s)
        if (ch >= 0x80) return false;
    return true;
}

}  // namespace

namespace flockgpu {

bool text_slice_streams(const SliceSpec &spec) {
    switch (spec.fn) {
        case SliceFn::SplitPart: return spec.arg.size() == 1;
        case SliceFn::Left: case SliceFn::Right: return true;
        default: return all_ascii(spec.arg);
    }
}

int text_slice(flockgpu_ctx *ctx, const char *name, const DevColumn &col, int64_t rows, const SliceSpec &spec, const int32_t *in_begin, const int32_t *in_end,
               int32_t **out_begin, int32_t **out_end) {
    const std::string base = name;
    const int64_t n = std::max<int64_t>(rows, 0);
    int32_t *ob = nullptr, *oe = nullptr;
    FG_TRY(arena_get_t(ctx, (base + ".b").c_str(), (size_t)n + 4, &ob));
    FG_TRY(arena_get_t(ctx, (base + ".e").c_str(), (size_t)n + 4, &oe));
    *out_begin = ob;
    *out_end = oe;
    if (n == 0) return FLOCKGPU_OK;
    if (n >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than 2^31 rows", name);
    if (col.type != ColType::UTF8 || !col.offsets) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: not a Utf8 column", name);
    if ((in_begin == nullptr) != (in_end == nullptr)) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: an inner slice needs both arrays", name);
    const uint8_t *bytes = static_cast<const uint8_t *>(col.values);
    if (!text_slice_streams(spec)) {
        GeneralParams P{};
        P.fn = (int32_t)spec.fn;
        P.n = spec.n;
        if (spec.fn == SliceFn::SplitPart) {
            if (spec.arg.empty() || spec.arg.size() > (size_t)kSliceMaxDelimBytes || spec.n <= 0) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: split_part delimiter / field outside its limits", name);
            P.len = (uint32_t)spec.arg.size();
            for (size_t k = 0; k < spec.arg.size(); ++k) P.v[k >> 2] |= (uint32_t)(uint8_t)spec.arg[k] << (8 * (k & 3));
        } else {
            for (size_t i = 0; i < spec.arg.size();) {   // a code point: a byte and the continuation bytes behind it (A-SL6)
                size_t l = 1;
                while (i + l < spec.arg.size() && ((uint8_t)spec.arg[i + l] & 0xc0u) == 0x80u) ++l;
                if (P.len >= (uint32_t)kSliceMaxTrimChars) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: more than %d trim characters", name, kSliceMaxTrimChars);
                if (l <= 4) {   // (a longer run is no code point of any value: code_point_at gives it the value nothing in the set has)
                    uint32_t v = 0;
                    for (size_t k = 0; k < l; ++k) v |= (uint32_t)(uint8_t)spec.arg[i + k] << (8 * k);
                    P.v[P.len++] = v;
                }
                i += l;
            }
        }
        const unsigned grid = (unsigned)std::min<int64_t>(div_up(n, kBlock), (int64_t)ctx->num_cus * 16);
        LaunchScope ls(ctx, "text_slice_general_kernel");
        hipLaunchKernelGGL(text_slice_general_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, col.offsets, bytes, n, in_begin, in_end, P, ob, oe);
        return check_launch(ctx, "text_slice_general_kernel");
    }
    StreamParams P{};
    const int32_t *krow = nullptr;
    int cls = kLead;
    const int64_t cnt = spec.n < 0 ? -(int64_t)spec.n : (int64_t)spec.n;   // |n|
    auto target = [](int64_t k) { return k >= (int64_t)kNever ? kNever : (uint32_t)k; };
    auto per_row = [&](int to) {   // k = the row's code points - |n|
        int32_t *len = nullptr;
        FG_TRY(utf8_lengths(ctx, (base + ".cp").c_str(), col, n, true, &len, in_begin, in_end));
        krow = len;
        P.row_to = to;
        P.row_sub = cnt;
        return (int)FLOCKGPU_OK;
    };
    switch (spec.fn) {
        case SliceFn::SplitPart:
            if (spec.n <= 0) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: split_part field must be positive", name);
            cls = kEqual;
            P.delim = (uint8_t)spec.arg[0];
            P.kb = target(cnt - 1);
            P.ke = target(cnt);
            P.adj = 1;
            break;
        case SliceFn::Left:
            if (spec.n >= 0) P.ke = target(cnt + 1);
            else FG_TRY(per_row(2));
            break;
        case SliceFn::Right:
            if (spec.n == 0) P.kb = kNever;          // '': begin = the row's end
            else if (spec.n < 0) P.kb = target(cnt + 1);
            else FG_TRY(per_row(1));
            break;
        case SliceFn::Ltrim: case SliceFn::Rtrim: case SliceFn::Btrim:
            cls = kOutside;
            for (unsigned char ch : spec.arg) ascii_set_add(P.set, ch);
            if (spec.fn != SliceFn::Rtrim) P.kb = 1;
            if (spec.fn != SliceFn::Ltrim) P.last = 1;
            break;
    }
    const dim3 grid((unsigned)div_up(n, kSliceRows)), block(kBlock);
    LaunchScope ls(ctx, "text_slice_stream_kernel");
    if (cls == kLead) hipLaunchKernelGGL(text_slice_stream_kernel<kLead>, grid, block, 0, ctx->stream, col.offsets, bytes, n, in_begin, in_end, krow, P, ob, oe);
    else if (cls == kEqual) hipLaunchKernelGGL(text_slice_stream_kernel<kEqual>, grid, block, 0, ctx->stream, col.offsets, bytes, n, in_begin, in_end, krow, P, ob, oe);
    else hipLaunchKernelGGL(text_slice_stream_kernel<kOutside>, grid, block, 0, ctx->stream, col.offsets, bytes, n, in_begin, in_end, krow, P, ob, oe);
    return check_launch(ctx, "text_slice_stream_kernel");
}

}  // namespace flockgpu
