// Aggregate window functions of WindowAggExec (relops.hpp window_aggregates): COUNT / SUM / MIN / MAX / AVG over the default frame, RANGE BETWEEN
// UNBOUNDED PRECEDING AND CURRENT ROW, on rows that arrive sorted by (PARTITION BY, ORDER BY).  Row i's value is the aggregate of its partition from the
// partition's first row through the LAST PEER of row i (equal ORDER BY values; without ORDER BY every row of the partition is a peer) -- a segmented
// inclusive scan whose value at the end of every peer group is broadcast back over the group.
//
// Three launches per pass of up to kMaxGroupAggs accumulators (reduce, then scan):
//   tile  : one workgroup per 2048-row tile (8 consecutive rows per lane).  Compares adjacent rows' keys once per node into two bit masks per lane
//           (partition starts, peer-group ends: 16 bits), and reduces the tile to two summaries: T, the segmented total from its last partition
//           start (or its first row) to its end, and H, the rows from its first row through its first peer-group end.  Later passes of the same
//           node read the bit masks instead of the keys.
//   carry : ONE workgroup walks the tile summaries: carry_in[t] (the scan's state before tile t: a partition may span every tile) and look[t],
//           the value at the first peer-group end after tile t -- what the rows of a peer group that runs on past the tile's end receive.  A
//           single-pass chained scan (decoupled look-back) would give the forward carry but not this look-ahead, which needs the LATER tiles' sums.
//   emit  : one workgroup per tile: the in-tile scan seeded with carry_in, the backward broadcast seeded with look, the finished columns
//           (Int32 narrowed, Float64 MIN / MAX mapped back, AVG divided) and their validity bytes.
// 16-byte loads and stores where the column's base is 16-byte aligned (every lane's 8 rows start at a multiple of 8 rows).  No host wait.
#include "orderkey.hpp"
#include "relops.hpp"
#include "scan.hpp"

namespace flockgpu {
namespace {

constexpr int kWinRows = 8;                       // consecutive rows per lane
constexpr int kWinTile = kBlock * kWinRows;       // 2048 rows per tile
constexpr int kCarryBlock = 1024;
constexpr int kWinMaxKeys = 8;                    // PARTITION BY + ORDER BY columns

enum WinOpCode : int32_t { W_COUNT = 0, W_SUM = 1, W_MAX_S = 2, W_MAX_U = 3, W_MIN_S = 4, W_MIN_U = 5 };
enum WinOutKind : int32_t { O_RAW64 = 0, O_I32 = 1, O_F64_ORD = 2, O_AVG = 3 };

struct WinKeys {
    const void *v[kWinMaxKeys];
    const uint8_t *valid[kWinMaxKeys];
    int32_t wide[kWinMaxKeys];   // 1: 64-bit storage, 0: Int32
    int32_t f64[kWinMaxKeys];    // Float64: compared through f64_canonical_bits (A-FO2 of relops.hpp: the zeros are one key, every NaN is one key)
    int32_t n_part, n_all;       // the first n_part columns are the PARTITION BY
};
struct WinAccs {
    const void *v[kMaxGroupAggs];          // null: COUNT
    const uint8_t *valid[kMaxGroupAggs];
    int32_t op[kMaxGroupAggs];
    int32_t wide[kMaxGroupAggs];
    int32_t f64[kMaxGroupAggs];            // Float64 MIN / MAX: the order-preserving bit pattern, compared unsigned
    int32_t vec;                           // 16-byte accesses allowed for every column of the pass
};
struct WinOuts {
    void *out[kMaxGroupAggs];
    uint8_t *valid[kMaxGroupAggs];   // null: no validity (COUNT)
    int32_t acc[kMaxGroupAggs];      // its accumulator (AVG: the count; the sum is acc + 1)
    int32_t kind[kMaxGroupAggs];
    int32_t n;
};

__device__ __forceinline__ uint64_t acc_identity(int32_t op) {
    switch (op) {
        case W_MAX_S: return 0x8000000000000000ull;
        case W_MIN_S: return 0x7fffffffffffffffull;
        case W_MIN_U: return ~0ull;
        default: return 0;
    }
}
__device__ __forceinline__ uint64_t acc_op(int32_t op, uint64_t a, uint64_t b) {
    switch (op) {
        case W_MAX_S: return (int64_t)a > (int64_t)b ? a : b;
        case W_MIN_S: return (int64_t)a < (int64_t)b ? a : b;
        case W_MAX_U: return a > b ? a : b;
        case W_MIN_U: return a < b ? a : b;
        default: return a + b;   // COUNT, SUM: two's complement
    }
}
__device__ __forceinline__ uint64_t f64_ord(uint64_t b) { return (b >> 63) ? ~b : (b | 0x8000000000000000ull); }
__device__ __forceinline__ uint64_t f64_unord(uint64_t o) { return (o >> 63) ? (o & 0x7fffffffffffffffull) : ~o; }

// A segment summary: f = a partition starts inside (the value then runs from the last start), v / vb = the accumulators and their "a valid value
// went in" bits.  comb(a, b), a the earlier: b when b holds a start, else a's values combined with b's.
template <int NA>
struct Seg {
    uint32_t f, vb;
    uint64_t v[NA];
};
template <int NA>
__device__ __forceinline__ Seg<NA> seg_identity(const WinAccs &A) {
    Seg<NA> s;
    s.f = 0;
    s.vb = 0;
#pragma unroll
    for (int a = 0; a < NA; ++a) s.v[a] = acc_identity(A.op[a]);
    return s;
}
template <int NA>
__device__ __forceinline__ Seg<NA> seg_comb(const WinAccs &A, const Seg<NA> &x, const Seg<NA> &y) {
    if (y.f) return y;
    Seg<NA> r;
    r.f = x.f;
    r.vb = x.vb | y.vb;
#pragma unroll
    for (int a = 0; a < NA; ++a) r.v[a] = acc_op(A.op[a], x.v[a], y.v[a]);
    return r;
}
// x's values combined with y's whatever the starts; f = y's (the head summaries: f = "holds a peer-group end")
template <int NA>
__device__ __forceinline__ Seg<NA> plain_comb(const WinAccs &A, const Seg<NA> &x, const Seg<NA> &y) {
    Seg<NA> r;
    r.f = y.f;
    r.vb = x.vb | y.vb;
#pragma unroll
    for (int a = 0; a < NA; ++a) r.v[a] = acc_op(A.op[a], x.v[a], y.v[a]);
    return r;
}
template <int NA>
__device__ __forceinline__ Seg<NA> seg_shfl_up(const Seg<NA> &s, int o) {
    Seg<NA> r;
    r.f = __shfl_up(s.f, o, 64);
    r.vb = __shfl_up(s.vb, o, 64);
#pragma unroll
    for (int a = 0; a < NA; ++a) r.v[a] = __shfl_up(s.v[a], o, 64);
    return r;
}
template <int NA>
__device__ __forceinline__ Seg<NA> seg_shfl_down(const Seg<NA> &s, int o) {
    Seg<NA> r;
    r.f = __shfl_down(s.f, o, 64);
    r.vb = __shfl_down(s.vb, o, 64);
#pragma unroll
    for (int a = 0; a < NA; ++a) r.v[a] = __shfl_down(s.v[a], o, 64);
    return r;
}
// inclusive segmented scan over the 64 lanes
template <int NA>
__device__ __forceinline__ Seg<NA> wave_seg_scan(const WinAccs &A, Seg<NA> s) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const Seg<NA> t = seg_shfl_up(s, o);
        if (lane_id() >= o) s = seg_comb(A, t, s);
    }
    return s;
}
// "first from the right": f = this lane's range holds a peer-group end, v / vb = the value at that end.  Lane l receives the nearest such value of
// lanes l + 1 .. 63 (f = 0 when none).
template <int NA>
__device__ __forceinline__ Seg<NA> wave_next_end(Seg<NA> s) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const Seg<NA> t = seg_shfl_down(s, o);
        if (lane_id() + o < 64 && !s.f) s = t;
    }
    Seg<NA> r = seg_shfl_down(s, 1);
    if (lane_id() == 63) r.f = 0;
    return r;
}

// 8 rows of a column from row r0 (r0 a multiple of 8) as 64-bit patterns (Int32 sign-extended); rows past n read 0
__device__ __forceinline__ void load8(const void *p, int32_t wide, int64_t r0, int64_t n, bool vec, uint64_t (&v)[kWinRows]) {
    if (vec && r0 + kWinRows <= n) {
        if (wide) {
            const uint4 *q = reinterpret_cast<const uint4 *>(static_cast<const uint64_t *>(p) + r0);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint4 t = q[k];
                v[2 * k] = (uint64_t)t.x | ((uint64_t)t.y << 32);
                v[2 * k + 1] = (uint64_t)t.z | ((uint64_t)t.w << 32);
            }
        } else {
            const int4 *q = reinterpret_cast<const int4 *>(static_cast<const int32_t *>(p) + r0);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int4 t = q[k];
                v[4 * k] = (uint64_t)(int64_t)t.x;
                v[4 * k + 1] = (uint64_t)(int64_t)t.y;
                v[4 * k + 2] = (uint64_t)(int64_t)t.z;
                v[4 * k + 3] = (uint64_t)(int64_t)t.w;
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < kWinRows; ++j) {
        const int64_t r = r0 + j;
        v[j] = r < n ? (wide ? static_cast<const uint64_t *>(p)[r] : (uint64_t)(int64_t) static_cast<const int32_t *>(p)[r]) : 0;
    }
}
__device__ __forceinline__ uint64_t load1(const void *p, int32_t wide, int64_t r) {
    return wide ? static_cast<const uint64_t *>(p)[r] : (uint64_t)(int64_t) static_cast<const int32_t *>(p)[r];
}
// validity of 8 rows as bits (null column: all valid); rows past n are 0
__device__ __forceinline__ uint32_t valid8(const uint8_t *p, int64_t r0, int64_t n, bool vec) {
    const uint32_t in_range = r0 + kWinRows <= n ? 0xffu : (r0 < n ? (1u << (uint32_t)(n - r0)) - 1u : 0u);
    if (!p) return in_range;
    uint32_t m = 0;
    if (vec && r0 + kWinRows <= n) {
        const uint2 w = *reinterpret_cast<const uint2 *>(p + r0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m |= ((w.x >> (8 * j)) & 0xffu) ? (1u << j) : 0u;
            m |= ((w.y >> (8 * j)) & 0xffu) ? (1u << (j + 4)) : 0u;
        }
        return m;
    }
#pragma unroll
    for (int j = 0; j < kWinRows; ++j)
        if (r0 + j < n && p[r0 + j]) m |= 1u << j;
    return m;
}

// Row flags of a lane: bits 0-7 partition starts, bits 8-15 peer-group ends of rows r0 .. r0 + 7 (rows past n: neither).  Two Float64 key values
// are the same key exactly when ORDER BY ties them (A-FO2, relops.hpp): the sort under the node interleaves -0.0 with +0.0 and NaNs of every pattern.
__device__ __forceinline__ uint32_t row_flags(const WinKeys &K, int64_t r0, int64_t n, bool vec) {
    if (r0 >= n) return 0;
    uint32_t pdiff = 0, gdiff = 0;   // bit k: row r0 + k (k = 0..8) differs from row r0 + k - 1 in a PARTITION BY / any key
    for (int c = 0; c < K.n_all; ++c) {
        uint64_t v[kWinRows];
        load8(K.v[c], K.wide[c], r0, n, vec, v);
        const uint32_t vm = valid8(K.valid[c], r0, n, vec);
        const bool has_prev = r0 > 0, has_next = r0 + kWinRows < n;
        uint64_t prev = has_prev ? load1(K.v[c], K.wide[c], r0 - 1) : 0, next = has_next ? load1(K.v[c], K.wide[c], r0 + kWinRows) : 0;
        if (K.f64[c]) {
#pragma unroll
            for (int k = 0; k < kWinRows; ++k) v[k] = f64_canonical_bits(v[k]);
            prev = f64_canonical_bits(prev);
            next = f64_canonical_bits(next);
        }
        const bool pv = has_prev && (!K.valid[c] || K.valid[c][r0 - 1]), nv = has_next && (!K.valid[c] || K.valid[c][r0 + kWinRows]);
        uint32_t d = 0;
#pragma unroll
        for (int k = 0; k <= kWinRows; ++k) {
            const uint64_t a = k < kWinRows ? v[k] : next, b = k > 0 ? v[k - 1] : prev;
            const bool va = k < kWinRows ? ((vm >> k) & 1u) : nv, vb = k > 0 ? ((vm >> (k - 1)) & 1u) : pv;
            if (va != vb || (va && a != b)) d |= 1u << k;
        }
        gdiff |= d;
        if (c < K.n_part) pdiff |= d;
    }
    if (r0 == 0) { pdiff |= 1u; gdiff |= 1u; }
    gdiff |= pdiff;
    const uint32_t in_range = r0 + kWinRows <= n ? 0xffu : (r0 < n ? (1u << (uint32_t)(n - r0)) - 1u : 0u);
    uint32_t gend = gdiff >> 1;                                            // row k ends its peer group when row k + 1 starts one ...
    if (r0 + kWinRows >= n && r0 < n) gend |= 1u << (uint32_t)(n - 1 - r0);   // ... or is the last row
    return (pdiff & in_range) | ((gend & in_range) << 8);
}

template <int NA>
__device__ __forceinline__ void load_accs(const WinAccs &A, int64_t r0, int64_t n, uint64_t (&v)[NA][kWinRows], uint32_t (&vm)[NA]) {
    const bool vec = A.vec != 0;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        vm[a] = valid8(A.valid[a], r0, n, vec);
        if (A.op[a] == W_COUNT) {
#pragma unroll
            for (int j = 0; j < kWinRows; ++j) v[a][j] = (vm[a] >> j) & 1u;
            continue;
        }
        load8(A.v[a], A.wide[a], r0, n, vec, v[a]);
        const uint64_t id = acc_identity(A.op[a]);
#pragma unroll
        for (int j = 0; j < kWinRows; ++j) {
            if (A.f64[a]) v[a][j] = f64_ord(v[a][j]);
            if (!((vm[a] >> j) & 1u)) v[a][j] = id;   // a NULL (or a row past the end) adds nothing
        }
    }
}

// The lane's T (from its last partition start) and H (from its first row through its first peer-group end) summaries
template <int NA>
__device__ __forceinline__ void lane_summaries(const WinAccs &A, uint32_t fl, const uint64_t (&v)[NA][kWinRows], const uint32_t (&vm)[NA], Seg<NA> *T, Seg<NA> *H) {
    *T = seg_identity<NA>(A);
    *H = seg_identity<NA>(A);
    bool head_open = true;
#pragma unroll
    for (int j = 0; j < kWinRows; ++j) {
        Seg<NA> r;
        r.f = (fl >> j) & 1u;
        r.vb = 0;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            r.v[a] = v[a][j];
            r.vb |= ((vm[a] >> j) & 1u) << a;
        }
        *T = seg_comb(A, *T, r);
        if (head_open) *H = seg_comb(A, *H, r);
        if ((fl >> (8 + j)) & 1u) head_open = false;
    }
    // H's f: the range holds a peer-group end.  (A partition start inside H can only be at its first row -- the row before any other start ends a
    // peer group -- and travels apart: bit 2 of the tile word.)
    H->f = (fl & 0xff00u) ? 1u : 0u;
}

// Tile summaries, tile-major: word[t] bit 0 T.f, bit 1 H.f (a peer-group end inside), bit 2 the tile's first row starts a partition, bits 8-11 T.vb,
// bits 12-15 H.vb; tv / hv [a * n_tiles + t].
template <int NA>
__global__ __launch_bounds__(kBlock) void win_tile_kernel(WinKeys K, WinAccs A, int64_t n, int32_t read_flags, uint16_t *__restrict__ flags,
                                                          uint32_t *__restrict__ word, uint64_t *__restrict__ tv, uint64_t *__restrict__ hv, int32_t n_tiles) {
    const int32_t tile = blockIdx.x;
    const int64_t r0 = (int64_t)tile * kWinTile + (int64_t)threadIdx.x * kWinRows;
    uint32_t fl;
    if (read_flags) {
        fl = flags[(size_t)tile * kBlock + threadIdx.x];
    } else {
        fl = row_flags(K, r0, n, A.vec != 0);
        flags[(size_t)tile * kBlock + threadIdx.x] = (uint16_t)fl;
    }
    uint64_t v[NA][kWinRows];
    uint32_t vm[NA];
    load_accs<NA>(A, r0, n, v, vm);
    Seg<NA> T, H;
    lane_summaries<NA>(A, fl, v, vm, &T, &H);
    const uint32_t hr = fl & 1u;   // the lane's first row starts a partition
    // wave reduction in lane order: T segmented; H = the first lane holding a peer-group end, everything before it combined plainly (no partition
    // starts there but at the range's first row)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const Seg<NA> t2 = seg_shfl_down(T, o), h2 = seg_shfl_down(H, o);
        if ((lane_id() & (2 * o - 1)) == 0) {
            if (!H.f) H = plain_comb(A, T, h2);   // (no peer-group end in the range: T = everything since its first row)
            T = seg_comb(A, T, t2);
        }
    }
    __shared__ Seg<NA> sT[kWavesPerBlock], sH[kWavesPerBlock];
    __shared__ uint32_t sR[kWavesPerBlock];
    if (lane_id() == 0) {
        sT[threadIdx.x >> 6] = T;
        sH[threadIdx.x >> 6] = H;
        sR[threadIdx.x >> 6] = hr;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Seg<NA> t = sT[0], h = sH[0];
        for (int w = 1; w < kWavesPerBlock; ++w) {
            if (!h.f) h = plain_comb(A, t, sH[w]);
            t = seg_comb(A, t, sT[w]);
        }
        word[tile] = (t.f ? 1u : 0u) | (h.f ? 2u : 0u) | (sR[0] ? 4u : 0u) | (t.vb << 8) | (h.vb << 12);
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            tv[(size_t)a * n_tiles + tile] = t.v[a];
            hv[(size_t)a * n_tiles + tile] = h.v[a];
        }
    }
}

template <int NA>
__device__ __forceinline__ Seg<NA> tile_T(const uint32_t *word, const uint64_t *tv, int32_t n_tiles, int32_t t) {
    Seg<NA> s;
    const uint32_t w = word[t];
    s.f = w & 1u;
    s.vb = (w >> 8) & 15u;
#pragma unroll
    for (int a = 0; a < NA; ++a) s.v[a] = tv[(size_t)a * n_tiles + t];
    return s;
}
// the value at tile t's first peer-group end, given the scan's state before the tile
template <int NA>
__device__ __forceinline__ Seg<NA> tile_end_value(const WinAccs &A, const Seg<NA> &cin, const uint32_t *word, const uint64_t *hv, int32_t n_tiles, int32_t t) {
    Seg<NA> h;
    const uint32_t w = word[t];
    h.f = (w >> 2) & 1u;   // the head starts a partition: the carry does not reach it
    h.vb = (w >> 12) & 15u;
#pragma unroll
    for (int a = 0; a < NA; ++a) h.v[a] = hv[(size_t)a * n_tiles + t];
    Seg<NA> r = seg_comb(A, cin, h);
    r.f = 1;
    return r;
}

// ONE workgroup: cin[t] = the scan's state before tile t, look[t] = the value at the first peer-group end after tile t (cw[t]: bits 0-3 / 4-7
// their validity)
template <int NA>
__global__ __launch_bounds__(kCarryBlock) void win_carry_kernel(WinAccs A, const uint32_t *__restrict__ word, const uint64_t *__restrict__ tv,
                                                                const uint64_t *__restrict__ hv, int32_t n_tiles, uint32_t *__restrict__ cw,
                                                                uint64_t *__restrict__ cin, uint64_t *__restrict__ look) {
    constexpr int kW = kCarryBlock / 64;
    const int32_t per = (n_tiles + kCarryBlock - 1) / kCarryBlock;
    const int32_t t0 = (int32_t)threadIdx.x * per, t1 = min(n_tiles, t0 + per);
    Seg<NA> s = seg_identity<NA>(A);
    for (int32_t t = t0; t < t1; ++t) s = seg_comb(A, s, tile_T<NA>(word, tv, n_tiles, t));
    // exclusive scan of the lanes' chunks across the workgroup
    const Seg<NA> incl = wave_seg_scan(A, s);
    Seg<NA> ex = seg_shfl_up(incl, 1);
    if (lane_id() == 0) ex = seg_identity<NA>(A);
    __shared__ Seg<NA> sw[kW];
    __shared__ Seg<NA> sn[kW];
    if (lane_id() == 63) sw[threadIdx.x >> 6] = incl;
    __syncthreads();
    Seg<NA> before = seg_identity<NA>(A);
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) before = seg_comb(A, before, sw[w]);
    Seg<NA> carry = seg_comb(A, before, ex);
    carry.f = 0;
    // forward: carry-in of every tile; the value at each tile's first peer-group end goes to look[] for the backward walk
    Seg<NA> first_end;
    first_end.f = 0;
    for (int32_t t = t0; t < t1; ++t) {
        uint32_t w = carry.vb;
#pragma unroll
        for (int a = 0; a < NA; ++a) cin[(size_t)a * n_tiles + t] = carry.v[a];
        if (word[t] & 2u) {
            const Seg<NA> e = tile_end_value(A, carry, word, hv, n_tiles, t);
            w |= e.vb << 4;
#pragma unroll
            for (int a = 0; a < NA; ++a) look[(size_t)a * n_tiles + t] = e.v[a];
            if (!first_end.f) first_end = e;
        }
        cw[t] = w;
        carry = seg_comb(A, carry, tile_T<NA>(word, tv, n_tiles, t));
        carry.f = 0;
    }
    // backward: the nearest end value to the right of every chunk (lanes of this wave, then the later waves' first), then of every tile
    Seg<NA> nx = wave_next_end(first_end);
    if (lane_id() == 0) sn[threadIdx.x >> 6] = first_end.f ? first_end : nx;
    __syncthreads();
    if (!nx.f)
        for (int w = (int)(threadIdx.x >> 6) + 1; w < kW; ++w)
            if (sn[w].f) { nx = sn[w]; break; }
    for (int32_t t = t1 - 1; t >= t0; --t) {
        const uint32_t w = cw[t];
        Seg<NA> mine;
        if (word[t] & 2u) {
            mine.f = 1;
            mine.vb = (w >> 4) & 15u;
#pragma unroll
            for (int a = 0; a < NA; ++a) mine.v[a] = look[(size_t)a * n_tiles + t];
        }
        cw[t] = (w & 15u) | ((nx.f ? nx.vb : 0u) << 4);
#pragma unroll
        for (int a = 0; a < NA; ++a) look[(size_t)a * n_tiles + t] = nx.f ? nx.v[a] : acc_identity(A.op[a]);
        if (word[t] & 2u) nx = mine;
    }
}

// One workgroup per tile: the finished window columns
template <int NA>
__global__ __launch_bounds__(kBlock) void win_emit_kernel(WinAccs A, WinOuts O, int64_t n, const uint16_t *__restrict__ flags, const uint32_t *__restrict__ cw,
                                                          const uint64_t *__restrict__ cin, const uint64_t *__restrict__ look, int32_t n_tiles) {
    const int32_t tile = blockIdx.x;
    const int64_t r0 = (int64_t)tile * kWinTile + (int64_t)threadIdx.x * kWinRows;
    const uint32_t fl = flags[(size_t)tile * kBlock + threadIdx.x];
    uint64_t v[NA][kWinRows];
    uint32_t vm[NA];
    load_accs<NA>(A, r0, n, v, vm);
    Seg<NA> T, H;
    lane_summaries<NA>(A, fl, v, vm, &T, &H);
    // forward: the state before this lane's first row
    const Seg<NA> incl = wave_seg_scan(A, T);
    Seg<NA> ex = seg_shfl_up(incl, 1);
    if (lane_id() == 0) ex = seg_identity<NA>(A);
    __shared__ Seg<NA> sw[kWavesPerBlock], sn[kWavesPerBlock];
    if (lane_id() == 63) sw[threadIdx.x >> 6] = incl;
    const uint32_t tw = cw[tile];
    Seg<NA> carry;
    carry.f = 0;
    carry.vb = tw & 15u;
#pragma unroll
    for (int a = 0; a < NA; ++a) carry.v[a] = cin[(size_t)a * n_tiles + tile];
    __syncthreads();
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) carry = seg_comb(A, carry, sw[w]);
    carry = seg_comb(A, carry, ex);
    // the in-lane inclusive scan
    uint64_t s[NA][kWinRows];
    uint32_t sb[kWinRows];
    Seg<NA> run = carry;
    run.f = 0;
#pragma unroll
    for (int j = 0; j < kWinRows; ++j) {
        const bool st = (fl >> j) & 1u;
        uint32_t b = st ? 0u : run.vb;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            run.v[a] = st ? v[a][j] : acc_op(A.op[a], run.v[a], v[a][j]);
            b |= ((vm[a] >> j) & 1u) << a;
            s[a][j] = run.v[a];
        }
        run.vb = b;
        sb[j] = b;
    }
    // backward: the value at the first peer-group end after this lane's rows
    Seg<NA> own;
    own.f = (fl & 0xff00u) ? 1u : 0u;
    own.vb = 0;
#pragma unroll
    for (int a = 0; a < NA; ++a) own.v[a] = 0;
#pragma unroll
    for (int j = kWinRows - 1; j >= 0; --j)
        if ((fl >> (8 + j)) & 1u) {
            own.vb = sb[j];
#pragma unroll
            for (int a = 0; a < NA; ++a) own.v[a] = s[a][j];
        }
    Seg<NA> nx = wave_next_end(own);
    if (lane_id() == 0) sn[threadIdx.x >> 6] = own.f ? own : nx;
    __syncthreads();
    if (!nx.f)
        for (int w = (int)(threadIdx.x >> 6) + 1; w < kWavesPerBlock; ++w)
            if (sn[w].f) { nx = sn[w]; break; }
    if (!nx.f) {   // the group runs on past the tile: its end value comes from the carry kernel
        nx.f = 1;
        nx.vb = (tw >> 4) & 15u;
#pragma unroll
        for (int a = 0; a < NA; ++a) nx.v[a] = look[(size_t)a * n_tiles + tile];
    }
#pragma unroll
    for (int j = kWinRows - 1; j >= 0; --j) {
        if ((fl >> (8 + j)) & 1u) {
            nx.vb = sb[j];
#pragma unroll
            for (int a = 0; a < NA; ++a) nx.v[a] = s[a][j];
        }
        sb[j] = nx.vb;
#pragma unroll
        for (int a = 0; a < NA; ++a) s[a][j] = nx.v[a];
    }
    // the columns
    if (r0 >= n) return;
    const bool full = A.vec && r0 + kWinRows <= n;
    for (int o = 0; o < O.n; ++o) {
        const int a = O.acc[o];
        uint64_t x[kWinRows];
        uint32_t ok = 0;
#pragma unroll
        for (int j = 0; j < kWinRows; ++j) {
            uint64_t val = 0;
            bool valid = true;
#pragma unroll
            for (int b = 0; b < NA; ++b)
                if (b == a) { val = s[b][j]; valid = (sb[j] >> b) & 1u; }
            if (O.kind[o] == O_AVG) {
                uint64_t sum = 0;
#pragma unroll
                for (int b = 0; b < NA; ++b)
                    if (b == a + 1) sum = s[b][j];
                const double d = val ? (double)(int64_t)sum / (double)val : 0.0;
                valid = val != 0;
                val = (uint64_t)__double_as_longlong(d);
            } else if (O.kind[o] == O_F64_ORD) {
                val = valid ? f64_unord(val) : 0;
            }
            if (!valid) val = 0;
            x[j] = val;
            ok |= (valid ? 1u : 0u) << j;
        }
        if (O.kind[o] == O_I32) {
            int32_t *p = static_cast<int32_t *>(O.out[o]);
            if (full) {
                int4 *q = reinterpret_cast<int4 *>(p + r0);
                q[0] = make_int4((int32_t)x[0], (int32_t)x[1], (int32_t)x[2], (int32_t)x[3]);
                q[1] = make_int4((int32_t)x[4], (int32_t)x[5], (int32_t)x[6], (int32_t)x[7]);
            } else {
                for (int j = 0; j < kWinRows && r0 + j < n; ++j) p[r0 + j] = (int32_t)x[j];
            }
        } else {
            uint64_t *p = static_cast<uint64_t *>(O.out[o]);
            if (full) {
                uint4 *q = reinterpret_cast<uint4 *>(p + r0);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    q[k] = make_uint4((uint32_t)x[2 * k], (uint32_t)(x[2 * k] >> 32), (uint32_t)x[2 * k + 1], (uint32_t)(x[2 * k + 1] >> 32));
            } else {
                for (int j = 0; j < kWinRows && r0 + j < n; ++j) p[r0 + j] = x[j];
            }
        }
        if (O.valid[o]) {
            uint8_t *p = O.valid[o];
            if (full) {
                uint2 w = make_uint2(0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    w.x |= ((ok >> j) & 1u) << (8 * j);
                    w.y |= ((ok >> (j + 4)) & 1u) << (8 * j);
                }
                *reinterpret_cast<uint2 *>(p + r0) = w;
            } else {
                for (int j = 0; j < kWinRows && r0 + j < n; ++j) p[r0 + j] = (uint8_t)((ok >> j) & 1u);
            }
        }
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int NA>
int launch_pass(flockgpu_ctx *ctx, const std::string &base, const WinKeys &K, const WinAccs &A, const WinOuts &O, int64_t rows, int32_t n_tiles,
                bool read_flags, uint16_t *flags) {
    uint32_t *word = nullptr, *cw = nullptr;
    uint64_t *tv = nullptr, *hv = nullptr, *cin = nullptr, *look = nullptr;
    FG_TRY(arena_get_t(ctx, (base + ".word").c_str(), (size_t)n_tiles + 4, &word));
    FG_TRY(arena_get_t(ctx, (base + ".cw").c_str(), (size_t)n_tiles + 4, &cw));
    FG_TRY(arena_get_t(ctx, (base + ".tv").c_str(), (size_t)NA * n_tiles + 4, &tv));
    FG_TRY(arena_get_t(ctx, (base + ".hv").c_str(), (size_t)NA * n_tiles + 4, &hv));
    FG_TRY(arena_get_t(ctx, (base + ".cin").c_str(), (size_t)NA * n_tiles + 4, &cin));
    FG_TRY(arena_get_t(ctx, (base + ".look").c_str(), (size_t)NA * n_tiles + 4, &look));
    {
        LaunchScope ls(ctx, "win_tile_kernel");
        hipLaunchKernelGGL(win_tile_kernel<NA>, dim3(n_tiles), dim3(kBlock), 0, ctx->stream, K, A, rows, read_flags ? 1 : 0, flags, word, tv, hv, n_tiles);
    }
    FG_TRY(check_launch(ctx, "win_tile_kernel"));
    {
        LaunchScope ls(ctx, "win_carry_kernel");
        hipLaunchKernelGGL(win_carry_kernel<NA>, dim3(1), dim3(kCarryBlock), 0, ctx->stream, A, word, tv, hv, n_tiles, cw, cin, look);
    }
    FG_TRY(check_launch(ctx, "win_carry_kernel"));
    {
        LaunchScope ls(ctx, "win_emit_kernel");
        hipLaunchKernelGGL(win_emit_kernel<NA>, dim3(n_tiles), dim3(kBlock), 0, ctx->stream, A, O, rows, flags, cw, cin, look, n_tiles);
    }
    return check_launch(ctx, "win_emit_kernel");
}

}  // namespace

int window_aggregates(flockgpu_ctx *ctx, const char *name, const DevColumn *keys, int n_part, int n_order, int64_t rows, const WinAgg *aggs, int n_aggs) {
    if (n_part < 0 || n_part > 4) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: PARTITION BY more than four columns", name);
    if (n_order < 0 || n_order > 4) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: window ORDER BY more than four columns", name);
    if (rows >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than 2^31 rows", name);
    if (rows <= 0 || n_aggs <= 0) return FLOCKGPU_OK;
    WinKeys K{};
    K.n_part = n_part;
    K.n_all = n_part + n_order;
    bool vec = true;
    for (int c = 0; c < K.n_all; ++c) {
        if (keys[c].type == ColType::UTF8) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: PARTITION BY / ORDER BY a Utf8 column", name);
        K.v[c] = keys[c].values;
        K.valid[c] = keys[c].valid;
        K.wide[c] = keys[c].type == ColType::I32 ? 0 : 1;
        K.f64[c] = keys[c].type == ColType::F64 ? 1 : 0;
        vec = vec && aligned16(keys[c].values) && aligned16(keys[c].valid);
    }
    for (int i = 0; i < n_aggs; ++i) {
        if (aggs[i].op != AggOp::COUNT && aggs[i].type == ColType::UTF8) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: a Utf8 argument", name);
        vec = vec && aligned16(aggs[i].values) && aligned16(aggs[i].valid) && aligned16(aggs[i].out) && aligned16(aggs[i].out_valid);
    }
    const std::string base = name;
    const int32_t n_tiles = (int32_t)((rows + kWinTile - 1) / kWinTile);
    uint16_t *flags = nullptr;
    FG_TRY(arena_get_t(ctx, (base + ".flags").c_str(), (size_t)n_tiles * kBlock + 8, &flags));
    // passes of up to kMaxGroupAggs accumulators (AVG takes two: its count and its sum); the first pass compares the keys, the others read its flags
    int i = 0, pass = 0;
    while (i < n_aggs) {
        WinAccs A{};
        WinOuts O{};
        int na = 0;
        A.vec = vec ? 1 : 0;
        while (i < n_aggs && na + (aggs[i].avg ? 2 : 1) <= kMaxGroupAggs) {
            const WinAgg &g = aggs[i];
            auto add = [&](AggOp op) {
                int32_t code = W_COUNT;
                switch (op) {
                    case AggOp::COUNT: code = W_COUNT; break;
                    case AggOp::SUM_INT: code = W_SUM; break;
                    case AggOp::MAX_S: code = W_MAX_S; break;
                    case AggOp::MIN_S: code = W_MIN_S; break;
                    case AggOp::MAX_U: case AggOp::MAX_F64: code = W_MAX_U; break;
                    case AggOp::MIN_U: case AggOp::MIN_F64: code = W_MIN_U; break;
                    default: code = -1;
                }
                A.op[na] = code;
                A.v[na] = op == AggOp::COUNT ? nullptr : g.values;
                A.valid[na] = g.valid;
                A.wide[na] = g.type == ColType::I32 ? 0 : 1;
                A.f64[na] = op == AggOp::MAX_F64 || op == AggOp::MIN_F64;
                return na++;
            };
            const int first = g.avg ? add(AggOp::COUNT) : add(g.op);
            if (A.op[first] < 0) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: accumulator %d is not a window accumulator", name, (int)g.op);
            if (g.avg) add(AggOp::SUM_INT);
            O.out[O.n] = g.out;
            O.valid[O.n] = g.out_valid;
            O.acc[O.n] = first;
            O.kind[O.n] = g.avg ? O_AVG : A.f64[first] ? O_F64_ORD : g.out_type == ColType::I32 ? O_I32 : O_RAW64;
            ++O.n;
            ++i;
        }
        const std::string pb = base + ".p" + std::to_string(pass);
        const bool rf = pass > 0;
        switch (na) {
            case 1: FG_TRY(launch_pass<1>(ctx, pb, K, A, O, rows, n_tiles, rf, flags)); break;
            case 2: FG_TRY(launch_pass<2>(ctx, pb, K, A, O, rows, n_tiles, rf, flags)); break;
            case 3: FG_TRY(launch_pass<3>(ctx, pb, K, A, O, rows, n_tiles, rf, flags)); break;
            default: FG_TRY(launch_pass<4>(ctx, pb, K, A, O, rows, n_tiles, rf, flags)); break;
        }
        ++pass;
    }
    return FLOCKGPU_OK;
}

}  // namespace flockgpu
