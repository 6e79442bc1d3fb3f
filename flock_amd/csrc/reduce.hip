// Ungrouped aggregates: the streaming pass and the fold (reduce.hpp).
#include "reduce.hpp"

#include <algorithm>
#include <string>

#include "scan.hpp"

using namespace flockgpu;

namespace {

constexpr uint64_t kSign64 = 0x8000000000000000ull;

// ---- combining two partials of one slot: the same operation in a lane, a wave, a workgroup and the fold
__device__ __forceinline__ uint64_t slot_merge(int32_t kind, uint64_t a, uint64_t b) {
    if (kind == (int32_t)ReduceKind::SumInt) return a + b;
    if (kind == (int32_t)ReduceKind::UMax) return a > b ? a : b;
    return (uint64_t)__double_as_longlong(__longlong_as_double((int64_t)a) + __longlong_as_double((int64_t)b));
}
__device__ __forceinline__ uint64_t wave_merge(int32_t kind, uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = slot_merge(kind, v, __shfl_xor(v, o, 64));
    return v;
}

// four validity bytes (one word) -> four bits
__device__ __forceinline__ uint32_t valid_nibble(uint32_t w) {
    const uint32_t nz = ((w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u;   // bit 8 j: byte j is not 0
    return (nz | (nz >> 7) | (nz >> 14) | (nz >> 21)) & 15u;
}
// validity of the lane's 32 rows of a tile inside the relation as bits (bit it * 4 + j): one aligned word per four rows
__device__ __forceinline__ uint32_t valid_bits_full(const uint8_t *__restrict__ valid, int64_t wbase) {
    if (!valid) return ~0u;
    uint32_t bits = 0;
#pragma unroll
    for (int it = 0; it < kFlagIters; ++it) bits |= valid_nibble(*reinterpret_cast<const uint32_t *>(valid + wbase + it * 256)) << (it * 4);
    return bits;
}

// The program is the kernels' FIRST argument and is read where the launch put it, in the kernel argument segment (scalar loads at uniform, computed
// offsets).  Indexing the by-value parameter itself with a loop counter makes the compiler copy it into scratch first -- 640 bytes per lane.
typedef const ReduceProgram __attribute__((address_space(4))) *ReduceProgramK;
__device__ __forceinline__ ReduceProgramK kernarg_program() { return (ReduceProgramK)__builtin_amdgcn_kernarg_segment_ptr(); }

// The slots' descriptors, read once per workgroup into (scalar) registers: inside the tile loop a descriptor fetched by slot number would be a dependent
// scalar load -- a round trip per slot and tile that nothing in the wave overlaps (a one-tile Final spent 40 us on them).
struct SlotRegs {
    uint32_t d[kReduceMaxSlots];      // col | kind << 8 | inv << 16 | f64 << 17; col 255: no slot
    uint64_t flip[kReduceMaxSlots];
};
__device__ __forceinline__ void load_slots(ReduceProgramK P, SlotRegs &r) {
#pragma unroll
    for (int k = 0; k < kReduceMaxSlots; ++k) {
        r.d[k] = k < P->n_slots ? ((uint32_t)P->slots[k].col | ((uint32_t)P->slots[k].kind << 8) | ((uint32_t)(P->slots[k].inv != 0) << 16) | ((uint32_t)(P->slots[k].f64 != 0) << 17)) : 255u;
        r.flip[k] = P->slots[k].flip;
    }
}

// A zero the compiler cannot see through.  What a slot does to a value starts from the mask bits and the value's sign, neither of which depends on
// the slot: left alone, the compiler computes all of it once, ahead of the loop over the slots -- per value, so a hundred registers stay live
// across that loop and spill.  OR-ing this zero in ties the work to the iteration that needs it.
__device__ __forceinline__ uint32_t opaque_zero() {
    uint32_t z;
    asm volatile("s_mov_b32 %0, 0" : "=s"(z));
    return z;
}

// The accumulators of column c over kIters groups of four values (mask bit it * 4 + j): straight-line code per value, the masked-off ones replaced
// by the slot's identity (0 in every kind: integer and Float64 sums add it, an order key is never below it).  The slot at work is picked out of
// the accumulators and put back by selects on the (uniform) slot number, so the array is indexed by constants only: registers, no scratch.
template <int kIters>
__device__ __forceinline__ void accumulate_i32(const SlotRegs &S, int n_slots, int c, uint32_t m_in, const int32_t (&v)[kIters][4], uint64_t (&acc)[kReduceMaxSlots]) {
#pragma unroll 1
    for (int a = 0; a < n_slots; ++a) {
        uint32_t d = 255u;
#pragma unroll
        for (int k = 0; k < kReduceMaxSlots; ++k) d = k == a ? S.d[k] : d;
        if ((int)(d & 255u) != c) continue;   // (uniform)
        const int32_t kind = (int32_t)((d >> 8) & 255u);
        uint64_t cur = 0;
#pragma unroll
        for (int k = 0; k < kReduceMaxSlots; ++k) cur = k == a ? acc[k] : cur;
        const uint32_t m = m_in | opaque_zero();
        if (kind == (int32_t)ReduceKind::SumInt) {
            int64_t s = (int64_t)cur;
#pragma unroll
            for (int it = 0; it < kIters; ++it)
#pragma unroll
                for (int j = 0; j < 4; ++j) s += (int64_t)v[it][j] * (int64_t)(int32_t)((m >> (it * 4 + j)) & 1u);
            cur = (uint64_t)s;
        } else {   // the order key of an Int32 in 32 bits; widened to the 64-bit key after the last tile
            const uint32_t flip = 0x80000000u ^ ((d >> 16) & 1u ? ~0u : 0u);
            uint32_t k = (uint32_t)cur;
#pragma unroll
            for (int it = 0; it < kIters; ++it)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t x = ((m >> (it * 4 + j)) & 1u) ? ((uint32_t)v[it][j] ^ flip) : 0u;
                    k = x > k ? x : k;
                }
            cur = k;
        }
#pragma unroll
        for (int k = 0; k < kReduceMaxSlots; ++k) acc[k] = k == a ? cur : acc[k];
    }
}
template <int kIters>
__device__ __forceinline__ void accumulate_u64(const SlotRegs &S, int n_slots, int c, uint32_t m_in, const uint64_t (&v)[kIters][4], uint64_t (&acc)[kReduceMaxSlots]) {
#pragma unroll 1
    for (int a = 0; a < n_slots; ++a) {
        uint32_t d = 255u;
#pragma unroll
        for (int k = 0; k < kReduceMaxSlots; ++k) d = k == a ? S.d[k] : d;
        if ((int)(d & 255u) != c) continue;   // (uniform)
        const int32_t kind = (int32_t)((d >> 8) & 255u);
        uint64_t cur = 0;
#pragma unroll
        for (int k = 0; k < kReduceMaxSlots; ++k) cur = k == a ? acc[k] : cur;
        const uint32_t m = m_in | opaque_zero();
        if (kind == (int32_t)ReduceKind::SumInt) {
            uint64_t s = cur;
#pragma unroll
            for (int it = 0; it < kIters; ++it)
#pragma unroll
                for (int j = 0; j < 4; ++j) s += ((m >> (it * 4 + j)) & 1u) ? v[it][j] : 0ull;
            cur = s;
        } else if (kind == (int32_t)ReduceKind::UMax) {
            uint64_t flip = 0;
#pragma unroll
            for (int k = 0; k < kReduceMaxSlots; ++k) flip = k == a ? S.flip[k] : flip;
            const uint64_t mag = (d >> 17) & 1u ? ~kSign64 : 0ull;
            const uint32_t z = opaque_zero();
            uint64_t k = cur;
#pragma unroll
            for (int it = 0; it < kIters; ++it)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint64_t b = v[it][j];
                    const uint64_t key = b ^ flip ^ ((uint64_t)(int64_t)((int32_t)((uint32_t)(b >> 32) | z) >> 31) & mag);
                    const uint64_t x = ((m >> (it * 4 + j)) & 1u) ? key : 0ull;
                    k = x > k ? x : k;
                }
            cur = k;
        } else {
            double s = __longlong_as_double((int64_t)cur);
#pragma unroll
            for (int it = 0; it < kIters; ++it)
#pragma unroll
                for (int j = 0; j < 4; ++j) s += ((m >> (it * 4 + j)) & 1u) ? __longlong_as_double((int64_t)v[it][j]) : 0.0;
            cur = (uint64_t)__double_as_longlong(s);
        }
#pragma unroll
        for (int k = 0; k < kReduceMaxSlots; ++k) acc[k] = k == a ? cur : acc[k];
    }
}

// One pass: workgroup b walks tiles b, b + G, ... of the flag-tile geometry (scan.hpp: 8192 rows, lane l of wave w holds rows w * 2048 + it * 256 +
// 4 l .. 4 l + 3).  A tile inside the relation: the column's eight 16-byte lane loads (eight at a time for a 64-bit column) are issued before the first value is used.  The
// relation's last, ragged tile goes four rows at a time, rows past the end reading the last row (and masked): no load sits under a per-row branch.
template <bool kMasked>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void global_reduce_kernel(const ReduceProgram program, int64_t n_rows, int32_t n_tiles, const uint32_t *__restrict__ flag_words,
                                                               uint64_t *__restrict__ slab) {
    const ReduceProgramK P = kernarg_program();
    __shared__ uint64_t s_red[kWavesPerBlock][kReduceMaxSlots + kReduceMaxCols];
    SlotRegs S;
    load_slots(P, S);
    const int n_slots = P->n_slots;
    uint64_t acc[kReduceMaxSlots];
    uint32_t cnt[kReduceMaxCols];
#pragma unroll
    for (int a = 0; a < kReduceMaxSlots; ++a) acc[a] = 0;
#pragma unroll
    for (int c = 0; c < kReduceMaxCols; ++c) cnt[c] = 0;

    for (int32_t tile = (int32_t)blockIdx.x; tile < n_tiles; tile += (int32_t)gridDim.x) {
        const int64_t wbase = (int64_t)tile * kFlagTile + flag_rel0();
        const bool full = (int64_t)(tile + 1) * kFlagTile <= n_rows;   // block-uniform
        const uint32_t rowmask = kMasked ? flag_words[(size_t)tile * kBlock + threadIdx.x] : ~0u;
#pragma unroll 1
        for (int c = 0; c < P->n_cols; ++c) {
            const void *values = P->cols[c].values;
            const uint8_t *valid = P->cols[c].valid;
            const bool is32 = P->cols[c].type == (int32_t)ColType::I32;
            uint32_t pc = 0;
            if (full) {
                const uint32_t m = rowmask & valid_bits_full(valid, wbase);
                pc = (uint32_t)__popc(m);
                if (is32) {
                    const int32_t *p = static_cast<const int32_t *>(values);
                    int32_t v[kFlagIters][4];
#pragma unroll
                    for (int it = 0; it < kFlagIters; ++it) {
                        const int4 t = stream_load4(p + wbase + it * 256);
                        v[it][0] = t.x; v[it][1] = t.y; v[it][2] = t.z; v[it][3] = t.w;
                    }
                    accumulate_i32<kFlagIters>(S, n_slots, c, m, v, acc);
                } else {
                    // (two halves of four 32-byte groups: 64 registers of values at a time would leave the accumulators none)
                    const uint64_t *p = static_cast<const uint64_t *>(values);
#pragma unroll 1
                    for (int h = 0; h < 2; ++h) {
                        uint64_t v[kFlagIters / 2][4];
#pragma unroll
                        for (int it = 0; it < kFlagIters / 2; ++it) {
                            const uint32_t *q = reinterpret_cast<const uint32_t *>(p + wbase + (h * (kFlagIters / 2) + it) * 256);
                            const uint4 lo = stream_load4u(q), hi = stream_load4u(q + 4);
                            v[it][0] = (uint64_t)lo.x | ((uint64_t)lo.y << 32);
                            v[it][1] = (uint64_t)lo.z | ((uint64_t)lo.w << 32);
                            v[it][2] = (uint64_t)hi.x | ((uint64_t)hi.y << 32);
                            v[it][3] = (uint64_t)hi.z | ((uint64_t)hi.w << 32);
                        }
                        accumulate_u64<kFlagIters / 2>(S, n_slots, c, m >> (h * 16), v, acc);
                    }
                }
            } else {
#pragma unroll 1
                for (int it = 0; it < kFlagIters; ++it) {
                    const int64_t r0 = wbase + it * 256, left = n_rows - r0;
                    if (!__ballot(left > 0)) continue;   // (wave-uniform: none of the wave's rows of this group exists -- a Final's few state rows are one group)
                    int64_t r[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) r[j] = j < left ? r0 + j : n_rows - 1;   // (n_rows >= 1: there is a tile)
                    uint32_t m4 = (rowmask >> (it * 4)) & (left >= 4 ? 15u : left <= 0 ? 0u : (1u << (int)left) - 1u);
                    if (valid) m4 &= valid_nibble((uint32_t)valid[r[0]] | ((uint32_t)valid[r[1]] << 8) | ((uint32_t)valid[r[2]] << 16) | ((uint32_t)valid[r[3]] << 24));
                    pc += (uint32_t)__popc(m4);
                    if (is32) {
                        const int32_t *p = static_cast<const int32_t *>(values);
                        const int32_t v[1][4] = {{p[r[0]], p[r[1]], p[r[2]], p[r[3]]}};
                        accumulate_i32<1>(S, n_slots, c, m4, v, acc);
                    } else {
                        const uint64_t *p = static_cast<const uint64_t *>(values);
                        const uint64_t v[1][4] = {{p[r[0]], p[r[1]], p[r[2]], p[r[3]]}};
                        accumulate_u64<1>(S, n_slots, c, m4, v, acc);
                    }
                }
            }
#pragma unroll
            for (int cc = 0; cc < kReduceMaxCols; ++cc) cnt[cc] += cc == c ? pc : 0u;
        }
    }
    // an Int32 column's 32-bit order keys -> the 64-bit keys of the sign-extended values (the identity maps to a key no value of the column is below)
#pragma unroll
    for (int a = 0; a < kReduceMaxSlots; ++a) {
        if (a >= P->n_slots || P->slots[a].kind != (int32_t)ReduceKind::UMax) continue;
        if (P->cols[P->slots[a].col].type != (int32_t)ColType::I32) continue;
        const uint32_t flip = 0x80000000u ^ (P->slots[a].inv ? ~0u : 0u);
        acc[a] = (uint64_t)(int64_t)(int32_t)((uint32_t)acc[a] ^ flip) ^ P->slots[a].flip;
    }
    // wave (shuffles) -> workgroup (LDS) -> this workgroup's row of the slab (plain stores; the fold launch reads them)
    const int wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int a = 0; a < kReduceMaxSlots; ++a) {
        if (a >= P->n_slots) continue;
        const uint64_t r = wave_merge(P->slots[a].kind, acc[a]);
        if (lane_id() == 0) s_red[wave][a] = r;
    }
#pragma unroll
    for (int c = 0; c < kReduceMaxCols; ++c) {
        if (c >= P->n_cols) continue;
        const uint64_t r = wave_sum_u64((uint64_t)cnt[c]);
        if (lane_id() == 0) s_red[wave][kReduceMaxSlots + c] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t *row = slab + (size_t)blockIdx.x * (P->n_slots + P->n_cols);   // (the slots, then the counts)
#pragma unroll
        for (int a = 0; a < kReduceMaxSlots; ++a) {
            if (a >= P->n_slots) continue;
            uint64_t r = s_red[0][a];
#pragma unroll
            for (int w = 1; w < kWavesPerBlock; ++w) r = slot_merge(P->slots[a].kind, r, s_red[w][a]);
            row[a] = r;
        }
#pragma unroll
        for (int c = 0; c < kReduceMaxCols; ++c) {
            if (c >= P->n_cols) continue;
            uint64_t r = 0;
#pragma unroll
            for (int w = 0; w < kWavesPerBlock; ++w) r += s_red[w][kReduceMaxSlots + c];
            row[P->n_slots + c] = r;
        }
    }
}

// The fold: ONE workgroup of 1024 merges the slab's rows (and sums the predicate pass's wave counts, four to a load, into the selected-row count), then
// thread 0 finishes the result row: decoded values, AVG's division, the Partial state layout, a validity byte per output.
constexpr int kFoldBlock = 1024;
constexpr int kFoldWaves = kFoldBlock / 64;
__global__ __launch_bounds__(kFoldBlock) void global_fold_kernel(const ReduceProgram program, const uint64_t *__restrict__ slab, int32_t n_slab_rows, const uint32_t *__restrict__ wave_counts,
                                                                 int64_t n_count_tiles, uint64_t rows_unmasked, uint64_t *__restrict__ out_values, uint8_t *__restrict__ out_valid) {
    const ReduceProgramK P = kernarg_program();
    constexpr int kW = kReduceMaxSlots + kReduceMaxCols;
    __shared__ uint64_t s_red[kFoldWaves][kW + 1];
    __shared__ uint64_t s_fin[kW + 1];
    uint64_t acc[kReduceMaxSlots], cnt[kReduceMaxCols], sel = 0;
#pragma unroll
    for (int a = 0; a < kReduceMaxSlots; ++a) acc[a] = 0;
#pragma unroll
    for (int c = 0; c < kReduceMaxCols; ++c) cnt[c] = 0;
    const int stride = P->n_slots + P->n_cols;
    for (int32_t g = (int32_t)threadIdx.x; g < n_slab_rows; g += kFoldBlock) {
        const uint64_t *row = slab + (size_t)g * stride;
#pragma unroll
        for (int a = 0; a < kReduceMaxSlots; ++a)
            if (a < P->n_slots) acc[a] = slot_merge(P->slots[a].kind, acc[a], row[a]);
#pragma unroll
        for (int c = 0; c < kReduceMaxCols; ++c)
            if (c < P->n_cols) cnt[c] += row[P->n_slots + c];
    }
    for (int64_t i = (int64_t)threadIdx.x; i < n_count_tiles; i += kFoldBlock) {   // (a tile's four wave counts: one 16-byte load)
        const uint4 w = *reinterpret_cast<const uint4 *>(wave_counts + i * kWavesPerBlock);
        sel += (uint64_t)w.x + w.y + w.z + w.w;
    }
    const int wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int a = 0; a < kReduceMaxSlots; ++a) {
        if (a >= P->n_slots) continue;
        const uint64_t r = wave_merge(P->slots[a].kind, acc[a]);
        if (lane_id() == 0) s_red[wave][a] = r;
    }
#pragma unroll
    for (int c = 0; c < kReduceMaxCols; ++c) {
        if (c >= P->n_cols) continue;
        const uint64_t r = wave_sum_u64(cnt[c]);
        if (lane_id() == 0) s_red[wave][kReduceMaxSlots + c] = r;
    }
    sel = wave_sum_u64(sel);
    if (lane_id() == 0) s_red[wave][kW] = sel;
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int a = 0; a < kReduceMaxSlots; ++a) {
        uint64_t r = 0;
        if (a < P->n_slots) {
            r = s_red[0][a];
#pragma unroll
            for (int w = 1; w < kFoldWaves; ++w) r = slot_merge(P->slots[a].kind, r, s_red[w][a]);
        }
        s_fin[a] = r;
    }
#pragma unroll
    for (int c = 0; c < kReduceMaxCols; ++c) {
        uint64_t r = 0;
        if (c < P->n_cols)
#pragma unroll
            for (int w = 0; w < kFoldWaves; ++w) r += s_red[w][kReduceMaxSlots + c];
        s_fin[kReduceMaxSlots + c] = r;
    }
    uint64_t rows = rows_unmasked;
    if (wave_counts) {
        rows = 0;
#pragma unroll
        for (int w = 0; w < kFoldWaves; ++w) rows += s_red[w][kW];
    }
    for (int o = 0; o < P->n_outs; ++o) {
        const struct { int32_t kind, col, a, b; } d = {P->outs[o].kind, P->outs[o].col, P->outs[o].a, P->outs[o].b};
        // (a column the node's input does not carry -- every value NULL -- has index -1: no value, count 0)
        const uint64_t n = d.col >= 0 ? s_fin[kReduceMaxSlots + d.col] : 0;
        const uint64_t va = d.a >= 0 ? s_fin[d.a] : 0, vb = d.b >= 0 ? s_fin[d.b] : 0;
        uint64_t val = 0;
        uint8_t ok = 1;
        switch (d.kind) {
            case (int32_t)ReduceOutKind::Rows: val = rows; break;
            case (int32_t)ReduceOutKind::ColCount: val = n; break;
            case (int32_t)ReduceOutKind::Value:
                ok = n != 0;
                if (d.a >= 0) {
                    const struct { int32_t kind, f64, inv; uint64_t flip; } s = {P->slots[d.a].kind, P->slots[d.a].f64, P->slots[d.a].inv, P->slots[d.a].flip};
                    if (s.kind != (int32_t)ReduceKind::UMax) {
                        val = va;
                    } else if (s.f64) {
                        const uint64_t k = va ^ (s.inv ? ~0ull : 0ull);
                        val = (k >> 63) ? (k & ~kSign64) : ~k;
                    } else {
                        val = va ^ s.flip;
                    }
                }
                break;
            case (int32_t)ReduceOutKind::ValueAlways: val = va; break;
            case (int32_t)ReduceOutKind::SumAsF64:
                val = (uint64_t)__double_as_longlong(d.b ? (double)va : (double)(int64_t)va);
                break;
            case (int32_t)ReduceOutKind::AvgOnePass:
                ok = n != 0;
                val = ok ? (uint64_t)__double_as_longlong((d.b ? (double)va : (double)(int64_t)va) / (double)n) : 0;
                break;
            default:   // AvgFinal
                ok = va != 0;
                val = ok ? (uint64_t)__double_as_longlong(__longlong_as_double((int64_t)vb) / (double)va) : 0;
                break;
        }
        out_values[o] = ok ? val : 0;
        out_valid[o] = ok;
    }
}

}  // namespace

namespace flockgpu {

int reduce_global(flockgpu_ctx *ctx, const char *name, const ReduceProgram &prog, int64_t rows, const uint32_t *flag_words, const uint32_t *wave_counts,
                  int32_t n_flag_tiles, uint64_t *out_values, uint8_t *out_valid) {
    if (prog.n_cols < 0 || prog.n_cols > kReduceMaxCols || prog.n_slots < 0 || prog.n_slots > kReduceMaxSlots || prog.n_outs < 1 || prog.n_outs > kReduceMaxOuts)
        return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: malformed reduce program", name);
    for (int a = 0; a < prog.n_slots; ++a)
        if (prog.slots[a].col < 0 || prog.slots[a].col >= prog.n_cols) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: a slot names a column the program does not have", name);
    for (int o = 0; o < prog.n_outs; ++o)
        if (prog.outs[o].col >= prog.n_cols || prog.outs[o].a >= prog.n_slots || (prog.outs[o].kind == (int32_t)ReduceOutKind::AvgFinal && prog.outs[o].b >= prog.n_slots))
            return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: an output names a slot or column the program does not have", name);
    if (rows < 0) rows = 0;
    if (rows >= (int64_t(1) << 44)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: too many rows", name);
    const bool masked = flag_words != nullptr;
    if (masked != (wave_counts != nullptr)) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: flag words without wave counts", name);
    const int32_t n_tiles = (int32_t)div_up(rows, (int64_t)kFlagTile);
    if (masked && n_flag_tiles != n_tiles) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: flag words of another relation", name);
    // (a node of counts of rows alone -- COUNT(*) -- streams nothing: over a filter the predicate pass's wave counts are its input)
    const int32_t grid = prog.n_cols > 0 ? (int32_t)std::min<int64_t>(n_tiles, (int64_t)ctx->num_cus * kReduceBlocksPerCu) : 0;
    uint64_t *slab = nullptr;
    FG_TRY(arena_get_t(ctx, (std::string(name) + ".slab").c_str(), (size_t)std::max(grid, 1) * (kReduceMaxSlots + kReduceMaxCols), &slab));
    if (grid > 0) {
        LaunchScope ls(ctx, "global_reduce_kernel");
        if (masked) hipLaunchKernelGGL((global_reduce_kernel<true>), dim3((unsigned)grid), dim3(kBlock), 0, ctx->stream, prog, rows, n_tiles, flag_words, slab);
        else hipLaunchKernelGGL((global_reduce_kernel<false>), dim3((unsigned)grid), dim3(kBlock), 0, ctx->stream, prog, rows, n_tiles, flag_words, slab);
    }
    FG_TRY(check_launch(ctx, "global_reduce_kernel"));
    {
        LaunchScope ls(ctx, "global_fold_kernel");
        hipLaunchKernelGGL(global_fold_kernel, dim3(1), dim3(kFoldBlock), 0, ctx->stream, prog, slab, grid, wave_counts, masked ? (int64_t)n_tiles : int64_t(0),
                           (uint64_t)rows, out_values, out_valid);
    }
    return check_launch(ctx, "global_fold_kernel");
}

}  // namespace flockgpu
