// UnionExec's column kernels (union.hpp): the inputs' values, validity bytes, Utf8 offsets and Utf8 bytes one after the other.
// Every index is checked against the launch's output range [lo, hi); a source index is taken only for an output element that exists, so no lane
// reads behind a source's last element (Utf8 offsets: behind off[rows]).  The streaming copy reads the ALIGNED 16-byte words that hold its sixteen
// bytes: a word is loaded only when it holds a byte the chunk needs, so it lies in a page the source owns.  Output buffers are 16-byte aligned
// (arena buffers are) and asked for with 16 bytes of slack.
#include <algorithm>
#include <string>
#include <vector>

#include "union.hpp"

using namespace flockgpu;

namespace {

constexpr int kChunksPerLane = kUnionTileChunks / kBlock;   // 4
static_assert(kUnionTileChunks % kBlock == 0, "a workgroup's chunks are whole rounds of its lanes");

// sixteen bytes from p, whatever its alignment: the one or two aligned 16-byte words that hold them, funnel-shifted (all sixteen bytes exist)
__device__ __forceinline__ uint4 load16_shifted(const void *p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(a & ~uintptr_t(15));
    const uint32_t m = (uint32_t)(a & 15);
    const uint4 w0 = stream_load4u(q);
    if (m == 0) return w0;
    const uint4 w1 = stream_load4u(q + 4);
    const uint32_t sh = 8 * (m & 3);
    uint32_t d0, d1, d2, d3, d4;
    switch (m >> 2) {   // (uniform over the lanes of one source: every chunk of it sits at the same misalignment)
        case 0: d0 = w0.x; d1 = w0.y; d2 = w0.z; d3 = w0.w; d4 = w1.x; break;
        case 1: d0 = w0.y; d1 = w0.z; d2 = w0.w; d3 = w1.x; d4 = w1.y; break;
        case 2: d0 = w0.z; d1 = w0.w; d2 = w1.x; d3 = w1.y; d4 = w1.z; break;
        default: d0 = w0.w; d1 = w1.x; d2 = w1.y; d3 = w1.z; d4 = w1.w; break;
    }
    return make_uint4(__funnelshift_r(d0, d1, sh), __funnelshift_r(d1, d2, sh), __funnelshift_r(d2, d3, sh), __funnelshift_r(d3, d4, sh));
}

enum class Mode { Values, Valid };
// what element i of source k gives.  Values: src[i], an all_null source (src null) zero.  Valid: valid[i], no validity bytes one, all_null zero.
template <typename T, Mode kMode>
__device__ __forceinline__ const T *source_ptr(const UnionSources &S, int k, T *konst) {
    const void *src = S.s[k].src;
    if (kMode == Mode::Values) {
        *konst = T(0);
        return static_cast<const T *>(src);
    }
    const uint8_t *valid = S.s[k].valid;
    *konst = src ? T(1) : T(0);
    return src ? reinterpret_cast<const T *>(valid) : nullptr;
}

// out[e] for the chunks of [S.lo, S.hi): element e of the output is element e - first of its source, through the source's row list where it has one.
template <typename T, Mode kMode>
__device__ __forceinline__ void union_chunks(const UnionSources &S, T *__restrict__ out) {
    constexpr uint32_t E = 16 / sizeof(T);
    const uint32_t chunk0 = S.lo / E, chunk_end = (S.hi + E - 1) / E;   // (hi <= 2^31)
#pragma unroll
    for (int r = 0; r < kChunksPerLane; ++r) {
        const uint32_t c = chunk0 + blockIdx.x * (uint32_t)kUnionTileChunks + (uint32_t)r * kBlock + threadIdx.x;
        if (c >= chunk_end) return;
        const uint32_t e0 = c * E;
        const bool whole = e0 >= S.lo && e0 + E <= S.hi;   // every element of the chunk is this launch's
        const uint32_t ef = max(e0, S.lo);                  // the first one that is
        int k = union_source_of(S, ef);
        uint32_t first = S.s[k].first, count = S.s[k].count;
        const int32_t *via = S.s[k].via;
        T konst;
        const T *src = source_ptr<T, kMode>(S, k, &konst);
        uint4 q;
        if (whole && union_seam_in_chunk(S, k, e0, E) == E && (!via || !src)) {
            // no seam inside: a constant, or the streaming copy at the source's alignment
            if (!src) {
                T v[E];
#pragma unroll
                for (uint32_t j = 0; j < E; ++j) v[j] = konst;
                __builtin_memcpy(&q, v, 16);
            } else {
                q = load16_shifted(src + (e0 - first));
            }
            stream_store4(out + e0, q);
            continue;
        }
        // a seam, a row list or the launch's edge: element by element, stepping to the next source where this one ends
        T v[E];
#pragma unroll
        for (uint32_t j = 0; j < E; ++j) {
            const uint32_t e = e0 + j;
            T x = T(0);
            if (e >= S.lo && e < S.hi) {
                while (e - first >= count) {   // (sources are non-empty and adjacent: e < hi ends the walk inside the table)
                    ++k;
                    first = S.s[k].first;
                    count = S.s[k].count;
                    via = S.s[k].via;
                    src = source_ptr<T, kMode>(S, k, &konst);
                }
                const uint32_t i = e - first;
                x = src ? src[via ? (uint32_t)via[i] : i] : konst;
            }
            v[j] = x;
        }
        if (whole) {
            __builtin_memcpy(&q, v, 16);
            stream_store4(out + e0, q);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < E; ++j)
                if (e0 + j >= S.lo && e0 + j < S.hi) out[e0 + j] = v[j];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void union_fixed_kernel(UnionSources S, T *__restrict__ out) {
    union_chunks<T, Mode::Values>(S, out);
}
__global__ __launch_bounds__(kBlock) void union_valid_kernel(UnionSources S, uint8_t *__restrict__ out) {
    union_chunks<uint8_t, Mode::Valid>(S, out);
}
// the sources' byte buffers one after the other: `first` / `count` are bytes, no row lists
__global__ __launch_bounds__(kBlock) void union_bytes_kernel(UnionSources S, uint8_t *__restrict__ out) {
    union_chunks<uint8_t, Mode::Values>(S, out);
}

// Utf8 offsets: entry e of [S.lo, S.hi) = the bytes in front of its source + the source's own entry e - first (an all_null source: empty strings);
// the launch that ends the column (`total_at` = S.hi) also writes entry S.hi, the byte total.  64-bit sums, narrowed: A-U6 was checked by the host.
__global__ __launch_bounds__(kBlock) void union_offsets_kernel(UnionSources S, uint64_t total, uint32_t write_total, int32_t *__restrict__ out_off) {
    const uint32_t end = S.hi + (write_total ? 1u : 0u);   // (hi < 2^31)
    const uint32_t chunk0 = S.lo / 4, chunk_end = (end + 3) / 4;
#pragma unroll
    for (int r = 0; r < kChunksPerLane; ++r) {
        const uint32_t c = chunk0 + blockIdx.x * (uint32_t)kUnionTileChunks + (uint32_t)r * kBlock + threadIdx.x;
        if (c >= chunk_end) return;
        const uint32_t e0 = c * 4;
        const bool whole = e0 >= S.lo && e0 + 4 <= end;
        const uint32_t ef = max(e0, S.lo);
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        if (ef < S.hi) {
            int k = union_source_of(S, ef);
            uint32_t first = S.s[k].first, count = S.s[k].count;
            const int32_t *off = static_cast<const int32_t *>(S.s[k].src);
            uint64_t base = S.base[k];
            if (whole && e0 + 4 <= S.hi && union_seam_in_chunk(S, k, e0, 4) == 4 && off) {
                const uint4 q = load16_shifted(off + (e0 - first));
                stream_store4(out_off + e0, make_uint4((uint32_t)union_rebased_offset(base, q.x), (uint32_t)union_rebased_offset(base, q.y),
                                                       (uint32_t)union_rebased_offset(base, q.z), (uint32_t)union_rebased_offset(base, q.w)));
                continue;
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t e = e0 + j;
                if (e >= S.lo && e < S.hi) {
                    while (e - first >= count) {
                        ++k;
                        first = S.s[k].first;
                        count = S.s[k].count;
                        off = static_cast<const int32_t *>(S.s[k].src);
                        base = S.base[k];
                    }
                    v[j] = (uint32_t)union_rebased_offset(base, off ? (uint64_t)(uint32_t)off[e - first] : 0);
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (write_total && e0 + j == S.hi) v[j] = (uint32_t)total;
        if (whole) {
            stream_store4(out_off + e0, make_uint4(v[0], v[1], v[2], v[3]));
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (e0 + j >= S.lo && e0 + j < end) out_off[e0 + j] = (int32_t)v[j];
        }
    }
}

enum class What { Fixed4, Fixed8, Valid, Bytes };
// the launches of one buffer: the sources in rounds of kUnionSources, each round its own output range
int launch_rounds(flockgpu_ctx *ctx, What what, const std::vector<UnionSource> &src, void *out) {
    const char *label = what == What::Valid ? "union_valid_kernel" : what == What::Bytes ? "union_bytes_kernel" : "union_fixed_kernel";
    const int64_t per = what == What::Fixed4 ? 4 : what == What::Fixed8 ? 2 : 16;   // elements of a chunk
    for (size_t r0 = 0; r0 < src.size(); r0 += (size_t)kUnionSources) {
        UnionSources S{};
        S.n = (int32_t)std::min<size_t>((size_t)kUnionSources, src.size() - r0);
        for (int i = 0; i < S.n; ++i) S.s[i] = src[r0 + (size_t)i];
        S.lo = S.s[0].first;
        S.hi = S.s[S.n - 1].first + S.s[S.n - 1].count;
        const int64_t chunks = div_up((int64_t)S.hi, per) - (int64_t)S.lo / per;
        const unsigned grid = (unsigned)div_up(chunks, kUnionTileChunks);
        {
            LaunchScope ls(ctx, label);
            if (what == What::Fixed4) hipLaunchKernelGGL(union_fixed_kernel<uint32_t>, dim3(grid), dim3(kBlock), 0, ctx->stream, S, static_cast<uint32_t *>(out));
            else if (what == What::Fixed8) hipLaunchKernelGGL(union_fixed_kernel<uint64_t>, dim3(grid), dim3(kBlock), 0, ctx->stream, S, static_cast<uint64_t *>(out));
            else if (what == What::Valid) hipLaunchKernelGGL(union_valid_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, S, static_cast<uint8_t *>(out));
            else hipLaunchKernelGGL(union_bytes_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, S, static_cast<uint8_t *>(out));
        }
        FG_TRY(check_launch(ctx, label));
    }
    return FLOCKGPU_OK;
}

}  // namespace

namespace flockgpu {

int union_column(flockgpu_ctx *ctx, const char *name, const UnionInput *in, int n_in, DevColumn *out) {
    const std::string base = name;
    if (n_in < 1) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: a union without inputs", name);
    const bool utf8 = in[0].col.type == ColType::UTF8;
    // (A-U6) rows and bytes, before anything is allocated
    std::vector<int64_t> rows((size_t)n_in), bytes((size_t)n_in, 0);
    bool any_valid = false, every_null = true, any_null = false;
    for (int k = 0; k < n_in; ++k) {
        if (in[k].col.type != in[0].col.type) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: input %d is of another type than input 0", name, k);
        if (utf8 && in[k].via) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: a Utf8 input arrives with a row list (it is taken first)", name);
        rows[(size_t)k] = std::max<int64_t>(in[k].rows, 0);
        every_null = every_null && in[k].col.all_null;
        if (rows[(size_t)k] == 0) continue;
        if (utf8 && !in[k].col.all_null) bytes[(size_t)k] = in[k].col.bytes;
        any_valid = any_valid || (in[k].col.valid && !in[k].col.all_null);
        any_null = any_null || in[k].col.all_null;
    }
    int64_t n = 0, out_bytes = 0;
    if (!union_rows_ok(rows.data(), n_in, &n)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than 2^31 rows", name);
    if (utf8 && !union_bytes_ok(bytes.data(), n_in, &out_bytes)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: Utf8 column exceeds 2^31 bytes", name);
    *out = in[0].col;
    out->valid = nullptr;
    out->offsets = nullptr;
    out->values = nullptr;
    out->bytes = 0;
    out->all_null = every_null;
    for (int k = 0; k < n_in; ++k) out->nullable = out->nullable || in[k].col.nullable;
    // the sources that have rows, in output order; bytes in front of each (Utf8)
    std::vector<UnionSource> src, bsrc;
    std::vector<uint64_t> front;
    int64_t at = 0, bat = 0;
    for (int k = 0; k < n_in; ++k) {
        if (rows[(size_t)k] == 0) continue;
        const DevColumn &c = in[k].col;
        UnionSource s{};
        s.src = c.all_null ? nullptr : (utf8 ? static_cast<const void *>(c.offsets) : c.values);
        s.via = in[k].via;
        s.valid = c.all_null ? nullptr : c.valid;
        s.first = (uint32_t)at;
        s.count = (uint32_t)rows[(size_t)k];
        if (!c.all_null && !s.src) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: input %d has rows and no values", name, k);
        src.push_back(s);
        front.push_back((uint64_t)bat);
        if (utf8 && bytes[(size_t)k] > 0) {
            UnionSource b{};
            b.src = c.values;
            b.first = (uint32_t)bat;
            b.count = (uint32_t)bytes[(size_t)k];
            if (!b.src) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: input %d has bytes and no buffer", name, k);
            bsrc.push_back(b);
        }
        at += rows[(size_t)k];
        bat += bytes[(size_t)k];
    }
    // (A-U3) validity bytes exactly when some input carries them -- or is nothing but NULLs beside inputs that are not
    if (!every_null && (any_valid || any_null)) {
        uint8_t *v = nullptr;
        FG_TRY(arena_get_t(ctx, (base + ".valid").c_str(), (size_t)n + 16, &v));
        FG_TRY(launch_rounds(ctx, What::Valid, src, v));
        out->valid = v;
    }
    if (!utf8) {
        void *pv = nullptr;
        const size_t w = col_width(in[0].col.type);
        FG_TRY(arena_get(ctx, (base + ".val").c_str(), (size_t)n * w + 16, &pv));
        FG_TRY(launch_rounds(ctx, w == 4 ? What::Fixed4 : What::Fixed8, src, pv));
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
    for (size_t r0 = 0; r0 < src.size(); r0 += (size_t)kUnionSources) {
        UnionSources S{};
        S.n = (int32_t)std::min<size_t>((size_t)kUnionSources, src.size() - r0);
        for (int i = 0; i < S.n; ++i) {
            S.s[i] = src[r0 + (size_t)i];
            S.base[i] = front[r0 + (size_t)i];
        }
        S.lo = S.s[0].first;
        S.hi = S.s[S.n - 1].first + S.s[S.n - 1].count;
        const bool last = r0 + (size_t)kUnionSources >= src.size();
        const int64_t chunks = div_up((int64_t)S.hi + (last ? 1 : 0), 4) - (int64_t)S.lo / 4;
        const unsigned grid = (unsigned)div_up(chunks, kUnionTileChunks);
        {
            LaunchScope ls(ctx, "union_offsets_kernel");
            hipLaunchKernelGGL(union_offsets_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, S, (uint64_t)out_bytes, last ? 1u : 0u, o_off);
        }
        FG_TRY(check_launch(ctx, "union_offsets_kernel"));
    }
    return launch_rounds(ctx, What::Bytes, bsrc, o_b);
}

}  // namespace flockgpu
