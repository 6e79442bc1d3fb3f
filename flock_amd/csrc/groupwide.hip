// GROUP BY with five to sixteen accumulators over dense group ids (groupwide.hpp), three launches: clear the cells, the pass, the finish.
//
// The pass follows dense_group_kernel's geometry (relops.hip): one workgroup of 256 lanes per tile of 8192 rows, a lane holds four consecutive rows
// per access (one 16-byte load of ids or Int32 values, two of 64-bit values, one 4-byte load of validity bytes), the tile's id range is taken first.
// The host turns the accumulator list into a PROGRAM: the distinct (values, validity) columns, each with the cells it feeds -- accumulators that
// agree in column and operation share a cell (q17's SUM(price) and the sum of AVG(price)), COUNT(col) IS the valid-row count of col's validity
// column, COUNT(*) and the counts of columns without validity are one row count.  q17: nine accumulators, four columns, seven cells.
//
// Cells are 64 bits and start at 0, the identity of every operation here: sums add; a minimum or maximum is the UNSIGNED MAXIMUM of an order key
// (signed: bits ^ sign bit; Float64: orderkey.hpp; a minimum: the complement), as in reduce.hpp; whether a group saw a valid value at all is not the
// cell's business but its validity column's count.  A row whose contribution is 0 sends no atomic (the NULLs of a CASE without ELSE).
//
// LDS: [cell][bin] 64-bit words, bins = wide_group_bins(n_specs): 448 for five to eight accumulators, 224 for nine to sixteen.  A program holds at
// most n_specs value cells and n_specs valid-row counts (every accumulator over a nullable column of its own -- the state columns a Final reads
// are all distinct): 16 x 8 x 448 = 32 x 8 x 224 = 56 KB per workgroup at the worst (two workgroups per CU of 160 KB), 12 KB for q17's Partial
// (7 cells x 8 x 224: eight workgroups per CU, the limit of 32 waves) and 16 KB for its Final (nine state columns without validity).  All below
// the 64 KB a launch gets without asking.  A tile whose ids span no more than the bins aggregates there and flushes one run of consecutive groups
// per cell with non-returning atomics; a wider tile sends its rows to the global cells directly.
//
// dense_group_kernel's hot-group shortcut is here in a per-access form: its fold registers live across a tile and are sized by a compile-time
// accumulator count, while this pass runs a host-built cell list.  Per access of 256 rows a wave elects the most frequent of three lanes' ids; the
// rows that carry it (at least eight) are folded per lane, reduced across the wave and handed over by one lane: one atomic per cell and access in
// place of up to 256 on ONE address.  The other rows of a lane are combined while their ids agree (ascending runs) before they reach an atomic.
// DESIGN.md section 3a has the readings with and without it.
#include "groupwide.hpp"

#include <algorithm>

#include "orderkey.hpp"

using namespace flockgpu;

namespace {

constexpr int kWideTile = 8192;
constexpr int kWideIters = kWideTile / (kBlock * 4);   // accesses of four rows per lane
constexpr int kMaxWideCells = kMaxWideAggs + kMaxWideCols + 1;   // value cells + valid-row counts + the row count (32 at most: a row count stands for a COUNT)
static_assert(kWideTile == kWavesPerBlock * 64 * 4 * kWideIters, "a tile is whole accesses of every lane");

// how a cell merges (bits 0-1) and how a row's value becomes its contribution (bit 2)
constexpr int32_t kAdd = 0, kUMax = 1, kFAdd = 2, kF64Key = 4;

struct WideCol {
    const void *values;     // null: the column only counts its valid rows
    const uint8_t *valid;   // null: every row valid
    int32_t wide;           // 64-bit values (else Int32, sign-extended)
    int32_t vec;            // bit 0: `values` takes 16-byte loads, bit 1: `valid` takes 4-byte loads
    int32_t vcell;          // the cell that counts this column's valid rows (-1: nobody asks)
    int32_t cell_begin, cell_end;
};
struct WideProgram {
    WideCol cols[kMaxWideCols];
    int32_t n_cols;
    int32_t n_cells;
    int32_t rows_cell;   // the cell that counts every row (-1: nobody asks)
    int32_t kind[kMaxWideCells];
    uint64_t mask[kMaxWideCells];   // kUMax: xor of the value (order key) -- sign bit, complement of a minimum
};
struct WideFinish {
    int32_t n;
    int32_t kind[kMaxWideAggs];    // WideOutKind
    int32_t cell[kMaxWideAggs], cell2[kMaxWideAggs];
    int32_t vcell[kMaxWideAggs];   // validity: this cell is not 0 (-1: none written)
    int32_t dec[kMaxWideAggs];     // Value: 0 as is, 1 xor mask, 2 Float64 from its order key xor mask
    int32_t i32[kMaxWideAggs];
    uint64_t mask[kMaxWideAggs];
    void *out[kMaxWideAggs];
    uint8_t *valid[kMaxWideAggs];
};

inline unsigned grid_for(flockgpu_ctx *ctx, int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(div_up(n, kBlock), (int64_t)ctx->num_cus * 16));
}

__global__ __launch_bounds__(kBlock) void wide_group_init_kernel(uint64_t *__restrict__ cells, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) cells[i] = 0;
}

__device__ __forceinline__ uint64_t wide_combine(int32_t kind, uint64_t x, uint64_t y) {
    switch (kind & 3) {
        case kAdd: return x + y;
        case kUMax: return x > y ? x : y;
        default: return (uint64_t)__double_as_longlong(__longlong_as_double((long long)x) + __longlong_as_double((long long)y));
    }
}
// (results unused: the atomics do not return)
__device__ __forceinline__ void wide_merge(uint64_t *cell, int32_t kind, uint64_t v) {
    switch (kind & 3) {
        case kAdd: atomicAdd(reinterpret_cast<unsigned long long *>(cell), (unsigned long long)v); break;
        case kUMax: atomicMax(reinterpret_cast<unsigned long long *>(cell), (unsigned long long)v); break;
        default: atomicAdd(reinterpret_cast<double *>(cell), __longlong_as_double((long long)v)); break;
    }
}

__global__ __launch_bounds__(kBlock) void wide_group_kernel(const int32_t *__restrict__ gid, int64_t n_rows, int64_t n_groups, WideProgram P, uint32_t bins,
                                                            uint64_t *__restrict__ g_cells) {
    extern __shared__ __attribute__((aligned(16))) uint64_t s_cells[];   // [n_cells][bins]
    __shared__ uint32_t s_red[2][kWavesPerBlock];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    for (uint32_t i = threadIdx.x; i < (uint32_t)P.n_cells * bins; i += kBlock) s_cells[i] = 0;
    // the tile's ids: wave w holds rows [t0 + w * 2048, + 2048), lane l of access it the four rows at + it * 256 + 4 l; -1: no row, or an id outside the cells
    const int64_t t0 = (int64_t)blockIdx.x * kWideTile + wave * (kWideTile / kWavesPerBlock) + lane * 4;
    int32_t g[kWideIters][4];
    uint32_t mn = 0xffffffffu, mx = 0;
#pragma unroll
    for (int it = 0; it < kWideIters; ++it) {
        const int64_t r0 = t0 + it * 256;
        int32_t k[4];
        if (r0 + 4 <= n_rows) {
            const int4 a = *reinterpret_cast<const int4 *>(gid + r0);   // (read again by nobody in this pass, but by the distinct counts beside it)
            k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) k[j] = r0 + j < n_rows ? gid[r0 + j] : -1;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = (uint64_t)(uint32_t)k[j] < (uint64_t)n_groups && k[j] >= 0;
            g[it][j] = in ? k[j] : -1;
            mn = in && (uint32_t)k[j] < mn ? (uint32_t)k[j] : mn;
            mx = in && (uint32_t)k[j] > mx ? (uint32_t)k[j] : mx;
        }
    }
    mn = ~wave_max_u32(~mn);
    mx = wave_max_u32(mx);
    if (lane == 0) {
        s_red[0][wave] = mn;
        s_red[1][wave] = mx;
    }
    __syncthreads();   // (also: the bins are cleared)
    uint32_t tmin = s_red[0][0], tmax = s_red[1][0];
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) {
        tmin = s_red[0][w] < tmin ? s_red[0][w] : tmin;
        tmax = s_red[1][w] > tmax ? s_red[1][w] : tmax;
    }
    if (tmin == 0xffffffffu) return;   // no live row in the tile (block-uniform)
    const bool in_lds = tmax - tmin < bins;   // block-uniform
    // a lane's four contributions to one cell: rows whose ids agree are combined, what is left and is not the identity goes to the cell
    auto emit = [&](int32_t cell, int32_t kind, const int32_t *gq, const uint64_t *x) {
        uint64_t acc = x[0];
        int32_t cur = gq[0];
#pragma unroll
        for (int j = 1; j <= 4; ++j) {
            if (j < 4 && gq[j] == cur) {
                acc = wide_combine(kind, acc, x[j]);
                continue;
            }
            if (acc != 0 && cur >= 0) {
                if (in_lds) wide_merge(&s_cells[(size_t)cell * bins + ((uint32_t)cur - tmin)], kind, acc);
                else wide_merge(&g_cells[(int64_t)cell * n_groups + cur], kind, acc);
            }
            if (j < 4) {
                cur = gq[j];
                acc = x[j];
            }
        }
    };
    // The wave's hot group, elected per access among three lanes' first rows (half of NEXMark's bids name one auction: 128 of an access's 256 rows
    // would meet in ONE cell): its rows are folded per lane, reduced across the wave and handed over by lane 0 -- one atomic per cell and access.
    auto emit_hot = [&](int32_t cell, int32_t kind, int32_t hot, const bool *is_hot, const uint64_t *x) {   // (wave-uniform: every lane takes part)
        uint64_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (is_hot[j]) v = wide_combine(kind, v, x[j]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t w = (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)v, o, 64) | ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64) << 32);
            v = wide_combine(kind, v, w);
        }
        if (lane == 0 && v != 0) {
            if (in_lds) wide_merge(&s_cells[(size_t)cell * bins + ((uint32_t)hot - tmin)], kind, v);
            else wide_merge(&g_cells[(int64_t)cell * n_groups + hot], kind, v);
        }
    };
#pragma unroll
    for (int it = 0; it < kWideIters; ++it) {
        const int64_t r0 = t0 + it * 256;
        if (__ballot(r0 < n_rows) == 0) continue;   // (wave-uniform; a lane past the end holds no live row and loads nothing)
        const bool full = r0 + 4 <= n_rows;
        int32_t hot = -1;
        {
            int best = 7;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int32_t cand = __builtin_amdgcn_readlane(g[it][0], c * 21);
                const int n = cand < 0 ? 0 : __popcll((unsigned long long)__ballot(g[it][0] == cand));
                if (n > best) {
                    best = n;
                    hot = cand;
                }
            }
        }
        int32_t gq[4];      // the rows that go to the cells on their own: the hot group's are taken out
        bool is_hot[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            is_hot[j] = hot >= 0 && g[it][j] == hot;
            gq[j] = is_hot[j] ? -1 : g[it][j];
        }
        uint64_t x[4];
        if (P.rows_cell >= 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = g[it][j] >= 0 ? 1 : 0;
            emit(P.rows_cell, kAdd, gq, x);
            if (hot >= 0) emit_hot(P.rows_cell, kAdd, hot, is_hot, x);
        }
        for (int c = 0; c < P.n_cols; ++c) {   // (uniform: the program is a kernel argument)
            const WideCol col = P.cols[c];
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) ok[j] = g[it][j] >= 0;
            if (col.valid) {
                uint32_t vb = 0;
                if (full && (col.vec & 2)) {
                    vb = *reinterpret_cast<const uint32_t *>(col.valid + r0);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) vb |= (r0 + j < n_rows && col.valid[r0 + j] ? 1u : 0u) << (8 * j);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) ok[j] = ok[j] && ((vb >> (8 * j)) & 0xffu) != 0;
                if (col.vcell >= 0) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) x[j] = ok[j] ? 1 : 0;
                    emit(col.vcell, kAdd, gq, x);
                    if (hot >= 0) emit_hot(col.vcell, kAdd, hot, is_hot, x);
                }
            }
            if (col.cell_begin == col.cell_end) continue;
            uint64_t raw[4];
            if (col.wide) {
                const uint64_t *p = static_cast<const uint64_t *>(col.values) + r0;
                if (full && (col.vec & 1)) {
                    const uint4 lo = stream_load4u(reinterpret_cast<const uint32_t *>(p)), hi = stream_load4u(reinterpret_cast<const uint32_t *>(p) + 4);
                    raw[0] = ((uint64_t)lo.y << 32) | lo.x;
                    raw[1] = ((uint64_t)lo.w << 32) | lo.z;
                    raw[2] = ((uint64_t)hi.y << 32) | hi.x;
                    raw[3] = ((uint64_t)hi.w << 32) | hi.z;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) raw[j] = r0 + j < n_rows ? p[j] : 0;
                }
            } else {
                const int32_t *p = static_cast<const int32_t *>(col.values) + r0;
                int32_t v[4];
                if (full && (col.vec & 1)) {
                    const int4 a = stream_load4(p);
                    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = r0 + j < n_rows ? p[j] : 0;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) raw[j] = (uint64_t)(int64_t)v[j];
            }
            for (int cell = col.cell_begin; cell < col.cell_end; ++cell) {
                const int32_t kind = P.kind[cell];
                const uint64_t mask = P.mask[cell];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    uint64_t v = raw[j];
                    if (kind & kF64Key) v = f64_order_key(__longlong_as_double((long long)v));
                    x[j] = ok[j] ? v ^ mask : 0;
                }
                emit(cell, kind, gq, x);
                if (hot >= 0) emit_hot(cell, kind, hot, is_hot, x);
            }
        }
    }
    if (!in_lds) return;
    __syncthreads();
    // one run of consecutive groups per cell: consecutive lanes, consecutive words
    const uint32_t span = tmax - tmin + 1;
    for (uint32_t i = threadIdx.x; i < (uint32_t)P.n_cells * span; i += kBlock) {
        const uint32_t cell = i / span, b = i - cell * span;
        const uint64_t v = s_cells[(size_t)cell * bins + b];
        if (v != 0) wide_merge(&g_cells[(int64_t)cell * n_groups + tmin + b], P.kind[cell], v);
    }
}

// the result columns from the cells, one lane per group
__global__ __launch_bounds__(kBlock) void wide_group_finish_kernel(const uint64_t *__restrict__ cells, int64_t n_groups, WideFinish F) {
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * kBlock)
        for (int o = 0; o < F.n; ++o) {
            const uint64_t a = cells[(int64_t)F.cell[o] * n_groups + g];
            const uint64_t b = F.cell2[o] >= 0 ? cells[(int64_t)F.cell2[o] * n_groups + g] : 0;
            uint64_t v;
            switch (F.kind[o]) {
                case (int32_t)WideOutKind::Value:
                    v = F.dec[o] == 0 ? a : F.dec[o] == 1 ? a ^ F.mask[o] : f64_from_order_key(a ^ F.mask[o]);
                    break;
                case (int32_t)WideOutKind::SumAsF64: v = (uint64_t)__double_as_longlong((double)(int64_t)a); break;
                case (int32_t)WideOutKind::AvgInt: v = (uint64_t)__double_as_longlong((double)(int64_t)b / (double)a); break;
                default: v = (uint64_t)__double_as_longlong(__longlong_as_double((long long)b) / (double)a); break;   // AvgF64
            }
            if (F.i32[o]) static_cast<int32_t *>(F.out[o])[g] = (int32_t)(int64_t)v;
            else static_cast<uint64_t *>(F.out[o])[g] = v;
            if (F.valid[o]) F.valid[o][g] = cells[(int64_t)F.vcell[o] * n_groups + g] != 0 ? 1 : 0;
        }
}

}  // namespace

namespace flockgpu {

int wide_group_bins(int n_specs) { return n_specs <= 8 ? 448 : 224; }

int group_by_ids_wide(flockgpu_ctx *ctx, const char *name, const int32_t *gid, int64_t rows, int64_t n_groups, const AggSpec *specs, int n_specs,
                      const WideOut *outs, int n_outs, WideGroupResult *out) {
    *out = WideGroupResult{};
    const std::string base = name;
    if (n_specs < 1 || n_specs > kMaxWideAggs) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than %d accumulators in one GROUP BY", name, kMaxWideAggs);
    if (n_outs < 1 || n_outs > kMaxWideAggs || rows < 0 || n_groups < 0 || n_groups > rows || rows >= (int64_t(1) << 31) || (rows > 0 && !gid))
        return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: a wide GROUP BY without ids, or with more result columns than accumulators", name);
    // ---- the program: distinct columns, the cells each feeds
    WideProgram P{};
    P.rows_cell = -1;
    struct CellDef { int32_t kind; uint64_t mask; };
    std::vector<CellDef> col_cells[kMaxWideCols];
    int col_cell_of[kMaxWideAggs], col_of[kMaxWideAggs];   // per accumulator: its place in its column's cell list (-1: a count)
    auto find_col = [&](const void *values, const uint8_t *valid, bool wide, bool values_matter) -> int {
        for (int c = 0; c < P.n_cols; ++c)
            if (P.cols[c].valid == valid && (!values_matter || (P.cols[c].values == values && (P.cols[c].wide != 0) == wide))) return c;
        if (P.n_cols == kMaxWideCols) return -1;
        WideCol &w = P.cols[P.n_cols];
        w.values = values_matter ? values : nullptr;
        w.valid = valid;
        w.wide = wide ? 1 : 0;
        w.vec = (w.values && reinterpret_cast<uintptr_t>(w.values) % 16 == 0 ? 1 : 0) | (valid && reinterpret_cast<uintptr_t>(valid) % 4 == 0 ? 2 : 0);
        w.vcell = -1;
        return P.n_cols++;
    };
    constexpr uint64_t kSign = 0x8000000000000000ull;
    // (the columns that carry values first: a COUNT(col) then finds its validity column among them)
    for (int a = 0; a < n_specs; ++a) {
        const AggSpec &s = specs[a];
        col_of[a] = col_cell_of[a] = -1;
        if (s.op == AggOp::COUNT) continue;
        if (!s.values || s.type == ColType::UTF8) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: an accumulator without an integer or Float64 argument", name);
        const bool f64 = s.type == ColType::F64;
        CellDef d{};
        switch (s.op) {
            case AggOp::SUM_INT: d = {kAdd, 0}; break;
            case AggOp::SUM_F64: d = {kFAdd, 0}; break;
            case AggOp::MAX_S: d = {kUMax, kSign}; break;
            case AggOp::MIN_S: d = {kUMax, ~kSign}; break;
            case AggOp::MAX_U: d = {kUMax, 0}; break;
            case AggOp::MIN_U: d = {kUMax, ~uint64_t(0)}; break;
            case AggOp::MAX_F64: d = {kUMax | kF64Key, 0}; break;
            default: d = {kUMax | kF64Key, ~uint64_t(0)}; break;   // MIN_F64
        }
        if (f64 != (s.op == AggOp::SUM_F64 || s.op == AggOp::MAX_F64 || s.op == AggOp::MIN_F64))
            return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: an integer accumulator over a Float64 column, or a Float64 one over integers", name);
        const int c = find_col(s.values, s.valid, s.type != ColType::I32, true);
        if (c < 0) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than %d distinct argument columns in one GROUP BY", name, kMaxWideCols);
        col_of[a] = c;
        for (size_t i = 0; i < col_cells[c].size(); ++i)
            if (col_cells[c][i].kind == d.kind && col_cells[c][i].mask == d.mask) col_cell_of[a] = (int)i;
        if (col_cell_of[a] < 0) {
            col_cell_of[a] = (int)col_cells[c].size();
            col_cells[c].push_back(d);
        }
    }
    for (int a = 0; a < n_specs; ++a) {
        if (!specs[a].valid) continue;
        const int c = find_col(nullptr, specs[a].valid, false, false);
        if (c < 0) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than %d distinct argument columns in one GROUP BY", name, kMaxWideCols);
        if (specs[a].op == AggOp::COUNT) col_of[a] = c;
    }
    for (int c = 0; c < P.n_cols; ++c) {
        P.cols[c].cell_begin = P.n_cells;
        for (const CellDef &d : col_cells[c]) {
            P.kind[P.n_cells] = d.kind;
            P.mask[P.n_cells] = d.mask;
            ++P.n_cells;
        }
        P.cols[c].cell_end = P.n_cells;
    }
    // the valid-row count of a validity column: one cell, fed by the first column that carries it
    auto vcell_of = [&](const uint8_t *valid) -> int {
        for (int c = 0; c < P.n_cols; ++c)
            if (P.cols[c].valid == valid) {
                if (P.cols[c].vcell < 0) {
                    P.kind[P.n_cells] = kAdd;
                    P.mask[P.n_cells] = 0;
                    P.cols[c].vcell = P.n_cells++;
                }
                return P.cols[c].vcell;
            }
        return -1;
    };
    int cell_of[kMaxWideAggs], vcell_of_acc[kMaxWideAggs];
    for (int a = 0; a < n_specs; ++a) {
        vcell_of_acc[a] = specs[a].valid ? vcell_of(specs[a].valid) : -1;
        if (specs[a].op != AggOp::COUNT) {
            cell_of[a] = P.cols[col_of[a]].cell_begin + col_cell_of[a];
        } else if (specs[a].valid) {
            cell_of[a] = vcell_of_acc[a];
        } else {
            if (P.rows_cell < 0) {
                P.kind[P.n_cells] = kAdd;
                P.mask[P.n_cells] = 0;
                P.rows_cell = P.n_cells++;
            }
            cell_of[a] = P.rows_cell;
        }
    }
    // ---- the finish
    WideFinish F{};
    F.n = n_outs;
    for (int o = 0; o < n_outs; ++o) {
        const WideOut &w = outs[o];
        const bool two = w.kind == WideOutKind::AvgInt || w.kind == WideOutKind::AvgF64;
        if (w.acc < 0 || w.acc >= n_specs || (two && (w.acc2 < 0 || w.acc2 >= n_specs)) || w.type == ColType::UTF8)
            return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: a result column of no accumulator", name);
        F.kind[o] = (int32_t)w.kind;
        F.cell[o] = cell_of[w.acc];
        F.cell2[o] = two ? cell_of[w.acc2] : -1;
        F.i32[o] = w.type == ColType::I32 ? 1 : 0;
        F.vcell[o] = w.validity == 2 ? cell_of[w.acc] : w.validity == 1 ? vcell_of_acc[w.acc] : -1;
        if (w.kind == WideOutKind::Value && specs[w.acc].op != AggOp::COUNT) {
            const int32_t k = P.kind[cell_of[w.acc]];
            F.dec[o] = (k & 3) != kUMax ? 0 : (k & kF64Key) ? 2 : 1;
            F.mask[o] = P.mask[cell_of[w.acc]];
        }
        if (F.i32[o]) {
            int32_t *p = nullptr;
            FG_TRY(arena_get_t(ctx, (base + ".o" + std::to_string(o)).c_str(), (size_t)n_groups + 4, &p));
            F.out[o] = p;
        } else {
            uint64_t *p = nullptr;
            FG_TRY(arena_get_t(ctx, (base + ".o" + std::to_string(o)).c_str(), (size_t)n_groups + 2, &p));
            F.out[o] = p;
        }
        if (F.vcell[o] >= 0) FG_TRY(arena_get_t(ctx, (base + ".v" + std::to_string(o)).c_str(), (size_t)n_groups + 16, &F.valid[o]));
        out->col[o] = F.out[o];
        out->valid[o] = F.valid[o];
    }
    if (n_groups == 0) return FLOCKGPU_OK;
    uint64_t *cells = nullptr;
    const int64_t n_words = (int64_t)P.n_cells * n_groups;
    FG_TRY(arena_get_t(ctx, (base + ".cells").c_str(), (size_t)n_words + 2, &cells));
    {
        LaunchScope ls(ctx, "wide_group_init_kernel");
        hipLaunchKernelGGL(wide_group_init_kernel, dim3(grid_for(ctx, n_words)), dim3(kBlock), 0, ctx->stream, cells, n_words);
    }
    FG_TRY(check_launch(ctx, "wide_group_init_kernel"));
    {
        const uint32_t bins = (uint32_t)wide_group_bins(n_specs);
        const size_t lds = (size_t)P.n_cells * bins * 8;   // at most 56 KB (the header comment)
        LaunchScope ls(ctx, "wide_group_kernel");
        hipLaunchKernelGGL(wide_group_kernel, dim3((unsigned)div_up(rows, kWideTile)), dim3(kBlock), lds, ctx->stream, gid, rows, n_groups, P, bins, cells);
    }
    FG_TRY(check_launch(ctx, "wide_group_kernel"));
    {
        LaunchScope ls(ctx, "wide_group_finish_kernel");
        hipLaunchKernelGGL(wide_group_finish_kernel, dim3(grid_for(ctx, n_groups)), dim3(kBlock), 0, ctx->stream, static_cast<const uint64_t *>(cells), n_groups, F);
    }
    FG_TRY(check_launch(ctx, "wide_group_finish_kernel"));
    return FLOCKGPU_OK;
}

}  // namespace flockgpu
