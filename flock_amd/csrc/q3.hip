// NEXMark q3 for gfx950: per ElementWise window (1-s epoch)
//   Filter(auction.category = 10)  JOIN  Filter(person.state = 'or' OR 'id' OR 'ca')  ON seller = p_id
//   -> Projection [name, city, state, a_id]
// (benchmarks/src/nexmark/query/q3.sql, q3_plan.fmt:1-6, flock/src/distributed_plan/planner.rs:152-171).
//
// All windows of a schedule run in a handful of launches, not a handful per epoch: a tile never straddles a
// window and every window owns a region of one global table, so per-epoch work of a few hundred KB does not become
// launch-latency bound (SURVEY.md section 7 "hard parts").  Every step is a plain streaming grid or
// count -> scan -> emit (scan.hpp); no workgroup waits on another one.
//   stats : exact [min, max] of p_id per window and whether the window's p_ids are strictly increasing
//   DENSE path (every window's p_ids strictly increasing -- hence unique -- and their range affordable; NEXMark ids
//   are dense and time-ordered): the join table is a direct-address array  table[p_id - min] = person row  per
//   window (a perfect hash: no probing, no atomics, 4 B per id, L2 / MALL resident)
//     build : persons -> state filter (byte compare on the Utf8 buffers) -> one plain store per surviving person
//     probe : auctions -> category filter -> one table load per surviving auction -> row flags (flag tiles)
//     emit  : flag words -> (auction_row, person_row, a_id) in auction order
//   GENERAL path (duplicate / unsorted / sparse p_ids): multimap keyed p_id (one 64-bit CAS slot {key, head row} +
//   chain array) built from the filtered persons; the probe counts, then emits, every matching pair.
//   take  : the three Utf8 columns of the matching persons (lengths -> scan -> offsets + bytes), one host
//           synchronisation for all three.
// DataFusion builds on the LEFT (auction) side; which side is hashed is unobservable in the result multiset,
// so the smaller, key-unique side is built here while duplicates on either side still produce every pair.
#include <algorithm>

#include "gather.hpp"
#include "hashtab.hpp"

using namespace flockgpu;

namespace {

constexpr int kMaxLits = 8;
struct Utf8Lits {  // literals of the `state = lit OR ...` chain, each <= 8 bytes
    uint64_t bytes[kMaxLits];
    uint32_t len[kMaxLits];
    int32_t n;
};

struct WinTable {
    int32_t base;     // min p_id of the window
    uint32_t range;   // max - min + 1 (0: the window has no persons)
    uint64_t off;     // offset of the window's entries in the table arena (windows with gaps in their ids)
    // A window whose ids have NO gaps (range = rows: NEXMark's persons, any id-ordered dense source) needs no table at all: person
    // p_id sits in row first_row + (p_id - base), and "the state filter keeps it" is one bit.  The bits are a plain bitmap over the
    // rows of the window's person tiles (1 KiB per tile, bit = row - first tile's begin): the build kernel's lanes hold four
    // consecutive rows each, eight lanes OR their nibbles into one word with three DPP steps and store it -- no atomics -- and the
    // whole relation's bits (2.4 MB for 2e7 persons) stay in L2 under the probe, whose lookups no longer go to HBM (1.32x the
    // algorithmic traffic with the 80 MB row table).
    int32_t first_row;   // gapless: the window's first person row
    int32_t first_tile;  // gapless: index of the window's first person tile (bit blocks are indexed by tile)
    uint32_t lead;       // gapless: first_row - (first_row & ~3): where the window starts inside its first tile
    uint32_t gapless;
};

// ---- build (both paths): flag-tile row layout, four consecutive persons per lane and iteration ---------------------
// Up to 8 bytes of a Utf8 value as a little-endian word, read through three aligned 4-byte words whose indices are
// clamped to the value's last word (no read past its end); all loads are unconditional so that the loads of
// the 32 rows of a lane overlap instead of queueing behind per-row branches.
__device__ __forceinline__ uint64_t utf8_head8(const uint8_t *__restrict__ data, int32_t b, uint32_t len) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(data) + (uint32_t)b;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(addr & ~uintptr_t(3));
    const uint32_t sh = (uint32_t)(addr & 3) * 8;
    const uint32_t last = len ? (uint32_t)(((addr & 3) + len - 1) >> 2) : 0u;
    const uint32_t w0 = w[0], w1 = w[min(1u, last)], w2 = w[min(2u, last)];
    const uint64_t lo = __funnelshift_r(w0, w1, sh), hi = __funnelshift_r(w1, w2, sh);
    const uint64_t v = lo | (hi << 32);
    return len >= 8 ? v : (v & ((1ull << (8 * len)) - 1));
}

// offsets[r], offsets[r + 1] through one 8-byte load (dword-aligned is all the hardware asks)
__device__ __forceinline__ int2 load_off_pair_q3(const int32_t *__restrict__ off, int64_t r) {
    int2 v;
    __builtin_memcpy(&v, off + r, 8);
    return v;
}

__device__ __forceinline__ bool lits_hit(uint64_t v, uint32_t len, const Utf8Lits &lits) {
    bool hit = false;
#pragma unroll
    for (int l = 0; l < kMaxLits; ++l) hit = hit || (l < lits.n && lits.len[l] == len && lits.bytes[l] == v);
    return hit;
}

// Per iteration a wave holds 256 CONSECUTIVE persons (lane l: rows 4l .. 4l+3), so their `state` offsets are one 16-byte load
// per lane and their bytes one contiguous range of the data buffer: the range is fetched with coalesced 16-byte loads into the
// wave's LDS slot and every row's value is read from there.  (Before: five dword loads of offsets per lane and three dependent
// dword loads per ROW -- 22 % of the HBM roofline.)  A range that does not fit the slot (long strings) and chunks that touch the
// column's ends take the per-row global loads.
constexpr int kWaveStageBytes = 4096;                      // 16 B per row on average
constexpr int kWaveStageWords = kWaveStageBytes / 4 + 8;   // + phase (< 16 B) and the words utf8_head8-style reads touch past a value

__device__ __forceinline__ uint64_t lds_head8(const uint32_t *w, uint32_t byte_pos, uint32_t len) {
    const uint32_t wi = byte_pos >> 2, sh = (byte_pos & 3) * 8;
    const uint32_t w0 = w[wi], w1 = w[wi + 1], w2 = w[wi + 2];
    const uint64_t lo = __funnelshift_r(w0, w1, sh), hi = __funnelshift_r(w1, w2, sh);
    const uint64_t v = lo | (hi << 32);
    return len >= 8 ? v : (v & ((1ull << (8 * len)) - 1));
}

// kInline (bits mode only): no layout kernel in front -- every workgroup derives its window's table from the window's first and last id
// itself (two loads), the window's first workgroup leaves it in `wins_out` for the probe and emit kernels, and `err` is a word of PINNED
// HOST memory the host zeroed before the launch (plain system-scope stores of 1: no memset node, no copy back).  A window whose ids
// have gaps (or are not increasing: the row check below) voids the call; the host then runs the general sequence.
__device__ __forceinline__ void raise_flag(uint32_t *flag, bool host_word) {
    if (host_word) __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else atomicOr(flag, 1u);
}
// kAnyOrder (row-table mode only, the RANGE path): the layout came from exact statistics, not from the windows' edges, and the persons
// may arrive in any order -- nothing to verify here; that no two persons of a window share an id is q3_table_unique_kernel's check.
template <bool kDense, bool kBits, bool kInline = false, bool kAnyOrder = false>
__global__ __launch_bounds__(kBlock) void q3_build_kernel(const int32_t *__restrict__ p_id,
                                                          const int32_t *__restrict__ state_off,
                                                          const uint8_t *__restrict__ state_data, int64_t n_rows, SegTiles st,
                                                          Utf8Lits lits, const WinTable *__restrict__ wins, int32_t *direct,
                                                          uint32_t *__restrict__ bits, uint64_t *tables, uint32_t cap, int32_t *next,
                                                          uint32_t *err, int y_shift, WinTable *__restrict__ wins_out) {
    // A relation of a few hundred tiles (2e6 persons at 1e8 events: 245) leaves most CUs without a workgroup, and one
    // workgroup walks its tile's eight iterations alone: blockIdx.y splits the iterations of a tile over 8 >> y_shift
    // workgroups (rows are independent: nothing is produced per tile).
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[kWavesPerBlock][kWaveStageWords];
    const TileRange tr = locate_tile(st, (int32_t)blockIdx.x, kFlagTile);
    const int64_t wbase = tr.tile_begin + flag_rel0();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    uint32_t *stage = s_stage[wave];
    WinTable wt{};
    if (kDense && !kInline) wt = wins[tr.seg];
    if (kInline) {
        const int64_t lo = st.seg_off[2 * tr.seg], hi = st.seg_off[2 * tr.seg + 1];   // (hi > lo: the window has a tile)
        const int32_t first = p_id[lo], last = p_id[hi - 1];
        const bool gapless = (int64_t)last - (int64_t)first + 1 == hi - lo;
        wt = WinTable{first, gapless ? (uint32_t)(hi - lo) : 0u, 0, (int32_t)lo, st.tile_first[tr.seg], (uint32_t)(lo - (lo & ~int64_t(3))), gapless ? 1u : 0u};
        if (threadIdx.x == 0) {
            if (!gapless) raise_flag(err, true);
            if ((int32_t)blockIdx.x == st.tile_first[tr.seg] && blockIdx.y == 0) wins_out[tr.seg] = wt;
        }
    }
    uint64_t *tab = kDense ? nullptr : tables + (size_t)tr.seg * cap;
    int32_t key[kFlagIters][4];
    if (y_shift >= 3) {
        load_flag_tile(p_id, n_rows, tr, key);
    } else {   // the iterations of the tile are split over blockIdx.y: load this workgroup's only (all eight were 4x the p_id traffic at y_shift 1)
#pragma unroll
        for (int it = 0; it < kFlagIters; ++it) {
            if ((it >> y_shift) == (int)blockIdx.y) load4_i32(p_id, wbase + it * 256, n_rows, key[it]);
            else key[it][0] = key[it][1] = key[it][2] = key[it][3] = 0;
        }
    }
    const uintptr_t data_addr = reinterpret_cast<uintptr_t>(state_data);
    const bool off_aligned = (reinterpret_cast<uintptr_t>(state_off) & 15) == 0;
#pragma unroll
    for (int it = 0; it < kFlagIters; ++it) {
        if ((it >> y_shift) != (int)blockIdx.y) continue;  // (block-uniform)
        const int64_t r0 = wbase + it * 256;
        const int64_t chunk0 = r0 - lane * 4;               // the wave's first row of this iteration
        // the id in front of the chunk (one address per wave; order check).  Clamped into the column: the chunks of a ragged last tile lie
        // past its end (rocgdb caught the unclamped load faulting on a 3600-row column in a fresh process)
        const int32_t before = kDense ? p_id[chunk0 > 0 ? (chunk0 - 1 < n_rows ? chunk0 - 1 : n_rows - 1) : 0] : 0;
        int32_t off[5];
        const bool inside = off_aligned && chunk0 >= 0 && chunk0 + 256 < n_rows;  // (wave-uniform) all 257 offsets exist
        if (inside) {
            const int4 o = *reinterpret_cast<const int4 *>(state_off + r0);  // r0 is a multiple of 4: 16-byte aligned
            off[0] = o.x; off[1] = o.y; off[2] = o.z; off[3] = o.w;
            const int32_t last = state_off[chunk0 + 256];   // (one address per wave)
            const int32_t nxt = __shfl_down(off[0], 1, 64);
            off[4] = lane == 63 ? last : nxt;
        } else {
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int64_t r = r0 + j;
                off[j] = state_off[r < 0 ? 0 : (r > n_rows ? n_rows : r)];
            }
        }
        const int32_t b0 = __builtin_amdgcn_readfirstlane(off[0]);
        const int32_t b1 = __builtin_amdgcn_readlane(off[4], 63);
        const uint32_t phase = (uint32_t)((data_addr + (uint32_t)b0) & 15);
        const bool staged = inside && b1 >= b0 && (uint32_t)(b1 - b0) + phase <= (uint32_t)kWaveStageBytes;  // (wave-uniform)
        if (staged) {
            // a 16-byte aligned chunk that holds at least one byte of the range never crosses a page: reading its tail is safe
            const uint32_t span = (uint32_t)(b1 - b0) + phase;
            const uint4 *src = reinterpret_cast<const uint4 *>((data_addr + (uint32_t)b0) & ~uintptr_t(15));
            for (uint32_t o = lane * 16; b1 > b0 && o < span; o += 64 * 16) *reinterpret_cast<uint4 *>(reinterpret_cast<uint8_t *>(stage) + o) = src[o >> 4];
            __builtin_amdgcn_wave_barrier();
        }
        uint32_t nib = 0;   // kBits: this lane's four filter bits at their place in the word of its 8-lane group
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t r = r0 + j;
            const bool in = r >= tr.lo && r < tr.hi;
            const uint32_t len = in ? (uint32_t)(off[j + 1] - off[j]) : 0u;
            uint64_t v;
            if (staged) v = lds_head8(stage, in ? (uint32_t)(off[j] - b0) + phase : 0u, len > 8 ? 8u : len);
            else v = utf8_head8(state_data, len ? off[j] : 0, len > 8 ? 8u : len);  // len 0: nothing is read past the buffer
            const bool hit = in && len <= 8 && lits_hit(v, len, lits);
            if (kDense) {
                // EVERY person of the window stores into its slot -- its row when the state filter keeps it, -1 otherwise -- so a window
                // whose ids have no gaps (range = rows) needs no fill pass; the table layout came from the window's first and last id
                // alone (q3_edge_layout_kernel), so "strictly increasing" is verified here: an id at or below its predecessor's, or
                // outside [first, last], flags the call and the host takes the general path (one synchronisation, as before).
                if (in) {
                    const uint32_t idx = (uint32_t)key[it][j] - (uint32_t)wt.base;
                    int32_t prev;
                    if (j > 0) prev = key[it][j - 1];
                    else {
                        prev = __shfl_up(key[it][3], 1, 64);
                        if (lane == 0) prev = before;
                    }
                    const bool ordered = kAnyOrder || r == tr.lo || key[it][j] > prev;
                    if (idx < wt.range && ordered) {
                        if (!kBits) direct[wt.off + idx] = hit ? (int32_t)r : -1;
                    } else if (wt.range) {
                        raise_flag(err, kInline);   // (range 0: the layout pass declined the dense path already)
                    }
                }
                if (kBits) nib |= (hit ? 1u : 0u) << (4 * (lane & 7) + j);
            } else if (hit && !multimap_insert_marked(tab, cap, next, key[it][j], (int32_t)r)) {
                atomicOr(err, 1u);
            }
        }
        if (kDense && kBits) {   // 32 consecutive rows = 8 lanes = one word
            nib |= (uint32_t)__shfl_xor((int)nib, 1, 64);
            nib |= (uint32_t)__shfl_xor((int)nib, 2, 64);
            nib |= (uint32_t)__shfl_xor((int)nib, 4, 64);
            if ((lane & 7) == 0) bits[(size_t)blockIdx.x * (kFlagTile / 32) + wave * 64 + it * 8 + (lane >> 3)] = nib;
        }
        if (staged) __builtin_amdgcn_wave_barrier();  // the slot is rewritten by the next iteration
    }
}

// ---- dense probe: flags, then (auction_row, person_row, a_id) ----------------------------------------------------
// kBits: every window is gapless (bit blocks, no row table); else: the row table for every window.  Two instances, not a branch per
// window: both lookups unrolled over a lane's 32 rows in one kernel took 136 VGPRs (three waves per SIMD) and ran 20 % slower.
template <bool kBits>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void q3_probe_flag_kernel(const int32_t *__restrict__ seller,
                                                               const int32_t *__restrict__ category, int64_t n_rows,
                                                               int64_t category_lit, SegTiles st,
                                                               const WinTable *__restrict__ wins,
                                                               const int32_t *__restrict__ direct,
                                                               const uint32_t *__restrict__ bits,
                                                               uint32_t *__restrict__ flag_words,
                                                               uint32_t *__restrict__ counts) {
    int32_t tile = (int32_t)blockIdx.x;
    if (tile >= st.n_tiles) return;
    TileRange tr = locate_tile(st, tile, kFlagTile);
    const int32_t rel0 = flag_rel0();
#pragma unroll 1
    for (;;) {  // tiles b, b + G, ... with the next descriptor requested early (scan.hpp)
        int32_t s[kFlagIters][4], c[kFlagIters][4];
        load_flag_tile(seller, n_rows, tr, s);
        load_flag_tile(category, n_rows, tr, c);
        const WinTable wt = wins[tr.seg];
        const int32_t next = tile + (int32_t)gridDim.x;
        TileRange trn = tr;
        if (next < st.n_tiles) trn = locate_tile(st, next, kFlagTile);
        const int32_t rel_lo = (int32_t)(tr.lo - tr.tile_begin), rel_hi = (int32_t)(tr.hi - tr.tile_begin);
        const int32_t *tab = direct + wt.off;
        const uint32_t *wbits = bits + (size_t)wt.first_tile * (kFlagTile / 32);
        uint32_t flags = 0;
#pragma unroll
        for (int it = 0; it < kFlagIters; ++it)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int32_t rel = rel0 + it * 256 + j;
                const uint32_t idx = (uint32_t)s[it][j] - (uint32_t)wt.base;
                const bool need = rel >= rel_lo && rel < rel_hi && (int64_t)c[it][j] == category_lit && idx < wt.range;
                // unconditional load from a clamped index: a load under a per-row branch is waited for before the
                // next row is looked at, i.e. one memory round trip per surviving row instead of one per tile
                bool f;
                if (kBits) {   // the person's bit: tile and position from its row offset inside the window
                    const uint32_t rel_w = need ? wt.lead + idx : 0u;
                    f = need & ((wbits[rel_w >> 5] >> (rel_w & 31u)) & 1u);
                } else {
                    f = need & (tab[need ? idx : 0u] >= 0);
                }
                flags |= (f ? 1u : 0u) << (it * 4 + j);
            }
        store_flags_and_counts(flags, tile, flag_words, counts);
        if (next >= st.n_tiles) break;
        tile = next;
        tr = trn;
    }
}

// The same pass for a relation of a few hundred tiles (6e6 auctions at 1e8 events: 733 tiles, 2.9 per CU -- one thin wave of workgroups
// whose eight serial iterations each wait for a seller load, then for the lookup behind it: 17.8 us for 48 MB, 34 % of the roofline).
// Sixteen waves per tile instead of four: quarter q = threadIdx.x / 256 of the workgroup takes iterations 2q and 2q + 1 of the
// flag-tile layout, i.e. byte q of every lane's flag word (a plain byte store), and the four quarters' wave counts meet in LDS.
template <bool kBits, int kParts>
__global__ __launch_bounds__(kParts * kBlock) void q3_probe_flag_small_kernel(const int32_t *__restrict__ seller,
                                                                         const int32_t *__restrict__ category, int64_t n_rows,
                                                                         int64_t category_lit, SegTiles st,
                                                                         const WinTable *__restrict__ wins,
                                                                         const int32_t *__restrict__ direct,
                                                                         const uint32_t *__restrict__ bits,
                                                                         uint32_t *__restrict__ flag_words,
                                                                         uint32_t *__restrict__ counts) {
    constexpr int kPer = kFlagIters / kParts;   // iterations of the flag-tile layout per part: bits kPer * 4 * part .. of every lane's flag word
    static_assert(kParts == 2 || kParts == 4, "two or four parts per tile");
    __shared__ uint32_t s_cnt[kParts][kWavesPerBlock];
    const int32_t tile = (int32_t)blockIdx.x;
    const TileRange tr = locate_tile(st, tile, kFlagTile);
    const int quarter = threadIdx.x >> 8, t = threadIdx.x & (kBlock - 1), wave = t >> 6, lane = t & 63;
    const int32_t rel0 = wave * kFlagWaveRows + lane * 4;
    const WinTable wt = wins[tr.seg];
    const int32_t rel_lo = (int32_t)(tr.lo - tr.tile_begin), rel_hi = (int32_t)(tr.hi - tr.tile_begin);
    const int32_t *tab = direct + wt.off;
    const uint32_t *wbits = bits + (size_t)wt.first_tile * (kFlagTile / 32);
    int32_t sv[kPer][4], cv[kPer][4];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int64_t r0 = tr.tile_begin + rel0 + (quarter * kPer + k) * 256;
        load4_i32(seller, r0, n_rows, sv[k]);
        load4_i32(category, r0, n_rows, cv[k]);
    }
    uint32_t flags = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t rel = rel0 + (quarter * kPer + k) * 256 + j;
            const uint32_t idx = (uint32_t)sv[k][j] - (uint32_t)wt.base;
            const bool need = rel >= rel_lo && rel < rel_hi && (int64_t)cv[k][j] == category_lit && idx < wt.range;
            bool f;
            if (kBits) {
                const uint32_t rel_w = need ? wt.lead + idx : 0u;
                f = need & ((wbits[rel_w >> 5] >> (rel_w & 31u)) & 1u);
            } else {
                f = need & (tab[need ? idx : 0u] >= 0);
            }
            flags |= (f ? 1u : 0u) << (k * 4 + j);
        }
    if (kParts == 4) reinterpret_cast<uint8_t *>(flag_words)[((size_t)tile * kBlock + t) * 4 + quarter] = (uint8_t)flags;   // bits 8q .. 8q + 7 of the lane's word
    else reinterpret_cast<uint16_t *>(flag_words)[((size_t)tile * kBlock + t) * 2 + quarter] = (uint16_t)flags;           // bits 16q .. 16q + 15
    const uint32_t incl = wave_incl_scan_u32((uint32_t)__popc(flags));
    if (lane == 63) s_cnt[quarter][wave] = incl;
    __syncthreads();
    if (threadIdx.x < kWavesPerBlock) {
        uint32_t c = 0;
#pragma unroll
        for (int q = 0; q < kParts; ++q) c += s_cnt[q][threadIdx.x];
        counts[(size_t)tile * kWavesPerBlock + threadIdx.x] = c;
    }
}

// Workgroup shape of the few-tiles probe: sixteen waves per tile while all tiles' workgroups are resident at once (2048 threads per CU), else
// eight -- 733 tiles x 1024 threads (6e6 auctions) is 1.43 rounds of workgroups, i.e. a second, mostly empty round.
template <bool kBits>
static void launch_probe_small(flockgpu_ctx *ctx, int32_t n_tiles, const int32_t *seller, const int32_t *category, int64_t n_rows, int64_t category_lit,
                               const SegTiles &st, const WinTable *wins, const int32_t *direct, const uint32_t *bits, uint32_t *flag_words, uint32_t *counts) {
    if ((int64_t)n_tiles * 4 * kBlock <= (int64_t)ctx->num_cus * 2048)
        hipLaunchKernelGGL((q3_probe_flag_small_kernel<kBits, 4>), dim3((unsigned)n_tiles), dim3(4 * kBlock), 0, ctx->stream, seller, category, n_rows, category_lit, st, wins,
                           direct, bits, flag_words, counts);
    else
        hipLaunchKernelGGL((q3_probe_flag_small_kernel<kBits, 2>), dim3((unsigned)n_tiles), dim3(2 * kBlock), 0, ctx->stream, seller, category, n_rows, category_lit, st, wins,
                           direct, bits, flag_words, counts);
}

template <bool kBits>
__global__ __launch_bounds__(kBlock) void q3_emit_dense_kernel(const int32_t *__restrict__ seller,
                                                               const int32_t *__restrict__ a_id, SegTiles st,
                                                               const uint32_t *__restrict__ flag_words,
                                                               const uint32_t *__restrict__ counts,
                                                               const uint64_t *__restrict__ tile_base,
                                                               const WinTable *__restrict__ wins,
                                                               const int32_t *__restrict__ direct,
                                                               int32_t *__restrict__ out_auction_row,
                                                               int32_t *__restrict__ out_person_row,
                                                               int32_t *__restrict__ out_a_id) {
    __shared__ uint16_t s_list[kFlagTile];
    const int32_t tile = (int32_t)blockIdx.x;
    const uint4 wc = *reinterpret_cast<const uint4 *>(counts + (size_t)tile * kWavesPerBlock);
    if (wc.x + wc.y + wc.z + wc.w == 0) return;
    const uint32_t total = build_flag_list(flag_words[(size_t)tile * kBlock + threadIdx.x], wc, s_list);
    __syncthreads();
    const TileRange tr = locate_tile(st, tile, kFlagTile);
    const WinTable wt = wins[tr.seg];
    const uint64_t base = tile_base[tile];
    for (uint32_t i = threadIdx.x; i < total; i += kBlock) {
        const int64_t r = tr.tile_begin + s_list[i];
        stream_store(&out_auction_row[base + i], (int32_t)r);   // (results: not read again by this call except person_row, which the take reads once)
        const uint32_t idx = (uint32_t)(seller[r] - wt.base);
        out_person_row[base + i] = kBits ? wt.first_row + (int32_t)idx : direct[wt.off + idx];
        stream_store(&out_a_id[base + i], a_id[r]);
    }
}

// The same emit WITHOUT a scan launch in front of it (bits mode): the workgroup sums the lower tiles' counts itself
// (block_base_of_tile), the first tile of a window reports the window's output offset and the last tile the pair total -- straight into
// pinned host memory (h_off, h_info[1]) and, for the Utf8 take queued behind, into d_pairs.
__global__ __launch_bounds__(kBlock) void q3_emit_dense_self_kernel(const int32_t *__restrict__ seller, const int32_t *__restrict__ a_id, SegTiles st,
                                                                    const uint32_t *__restrict__ flag_words, const uint32_t *__restrict__ counts,
                                                                    const WinTable *__restrict__ wins, int32_t *__restrict__ out_auction_row,
                                                                    int32_t *__restrict__ out_person_row, int32_t *__restrict__ out_a_id,
                                                                    uint64_t *__restrict__ d_pairs, int64_t *__restrict__ h_off, uint64_t *__restrict__ h_info) {
    __shared__ uint16_t s_list[kFlagTile];
    __shared__ uint64_t s_red[kWavesPerBlock];
    const int32_t tile = (int32_t)blockIdx.x;
    const uint64_t base = block_base_of_tile(counts, tile, s_red);
    const uint4 wc = *reinterpret_cast<const uint4 *>(counts + (size_t)tile * kWavesPerBlock);
    const TileRange tr = locate_tile(st, tile, kFlagTile);
    if (threadIdx.x == 0) {
        if (tile == st.tile_first[tr.seg]) h_off[tr.seg] = (int64_t)base;
        if (tile == st.n_tiles - 1) {
            const uint64_t total = base + wc.x + wc.y + wc.z + wc.w;
            *d_pairs = total;
            h_info[1] = total;
        }
    }
    if (wc.x + wc.y + wc.z + wc.w == 0) return;
    const uint32_t total = build_flag_list(flag_words[(size_t)tile * kBlock + threadIdx.x], wc, s_list);
    __syncthreads();
    const WinTable wt = wins[tr.seg];
    for (uint32_t i = threadIdx.x; i < total; i += kBlock) {
        const int64_t r = tr.tile_begin + s_list[i];
        stream_store(&out_auction_row[base + i], (int32_t)r);
        const uint32_t idx = (uint32_t)(seller[r] - wt.base);
        out_person_row[base + i] = wt.first_row + (int32_t)idx;
        stream_store(&out_a_id[base + i], a_id[r]);
    }
}

// ---- general probe: every (auction, person) pair of a key, counted then emitted in auction order ------------------
template <bool kEmit>
__global__ __launch_bounds__(kBlock) void q3_probe_general_kernel(const int32_t *__restrict__ seller,
                                                                  const int32_t *__restrict__ category,
                                                                  const int32_t *__restrict__ a_id, int64_t n_rows,
                                                                  int64_t category_lit, SegTiles st, const uint64_t *tables,
                                                                  uint32_t cap, const int32_t *__restrict__ next,
                                                                  uint32_t *counts, const uint64_t *__restrict__ tile_base,
                                                                  int32_t *__restrict__ out_auction_row,
                                                                  int32_t *__restrict__ out_person_row,
                                                                  int32_t *__restrict__ out_a_id, uint32_t *__restrict__ heads) {
    // heads[tile * 8192 + position in the tile]: what the COUNT pass found for every row -- the first link of its partners' chain, or
    // kNoHead -- so that the EMIT pass does not hash and probe again (it read seller, category and the tables a second time: 0.376 ms of
    // random lookups per 6e7 auctions, against 0.24 GB written here and read there, both coalesced)
    const int32_t tile = (int32_t)blockIdx.x;
    const TileRange tr = locate_tile(st, tile, kFlagTile);
    const uint64_t *tab = tables + (size_t)tr.seg * cap;
    uint32_t *tile_heads = heads + (size_t)tile * kFlagTile + flag_rel0();
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const int64_t wbase = tr.tile_begin + flag_rel0();
    uint64_t pos = 0;
    if (kEmit) {
        const uint4 wc = *reinterpret_cast<const uint4 *>(counts + (size_t)tile * kWavesPerBlock);
        if (wc.x + wc.y + wc.z + wc.w == 0) return;
        pos = tile_base[tile] + (wave > 0 ? wc.x : 0u) + (wave > 1 ? wc.y : 0u) + (wave > 2 ? wc.z : 0u);
    }
    // the FIRST probe of a lane's four rows of an iteration goes out together from clamped slots -- at the load factor the host sizes
    // for (<= 0.67 of the window's persons, half of whom the state filter drops) it settles most rows; what is left walks on row by row
    uint32_t wave_total = 0;
#pragma unroll 1
    for (int it = 0; it < kFlagIters; ++it) {
        const int64_t r0 = wbase + it * 256;
        uint32_t head[4];   // the chain's first link: row | "has a successor" (hashtab.hpp); kNoHead: no partner
        constexpr uint32_t kNoHead = 0xFFFFFFFFu;   // (never a link: row 2^31 - 1 does not exist)
        uint32_t mine = 0;
        if (kEmit) {
            const uint4 h = *reinterpret_cast<const uint4 *>(tile_heads + it * 256);
            head[0] = h.x; head[1] = h.y; head[2] = h.z; head[3] = h.w;
        } else {
            int32_t sv[kFlagIters][4], cv[kFlagIters][4];   // (only row `it` is used: the whole tile in registers ran 10-20 % slower)
            load4_i32(seller, r0, n_rows, sv[it]);
            load4_i32(category, r0, n_rows, cv[it]);
            uint32_t slot[4];
            uint64_t first[4];
            bool need[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t r = r0 + j;
                need[j] = r >= tr.lo && r < tr.hi && (int64_t)cv[it][j] == category_lit;
                slot[j] = slot_of((uint32_t)sv[it][j], cap);
                first[j] = tab[need[j] ? slot[j] : 0u];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                head[j] = kNoHead;
                if (!need[j]) continue;
                uint64_t cur = first[j];
                uint32_t sl = slot[j];
                for (uint32_t probe = 0, lim = probe_limit(cap); probe < lim; ++probe) {
                    if (cur == kEmpty64) break;
                    if ((int32_t)(cur >> 32) == sv[it][j]) {
                        head[j] = (uint32_t)cur;
                        break;
                    }
                    sl = (sl + 1 == cap) ? 0 : sl + 1;
                    cur = tab[sl];
                }
            }
            *reinterpret_cast<uint4 *>(tile_heads + it * 256) = make_uint4(head[0], head[1], head[2], head[3]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (head[j] != kNoHead)
                for (uint32_t c = head[j];; c = (uint32_t)next[c & kChainRow]) {
                    ++mine;
                    if (!(c & kChainMore)) break;
                }
        const uint32_t incl = wave_incl_scan_u32(mine);
        const uint32_t it_total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (kEmit && it_total) {
            uint64_t p = pos + (incl - mine);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (head[j] == kNoHead) continue;
                for (uint32_t c = head[j];; c = (uint32_t)next[c & kChainRow]) {
                    out_auction_row[p] = (int32_t)(r0 + j);
                    out_person_row[p] = (int32_t)(c & kChainRow);
                    out_a_id[p] = a_id[r0 + j];
                    ++p;
                    if (!(c & kChainMore)) break;
                }
            }
        }
        pos += it_total;
        wave_total += it_total;
    }
    if (!kEmit && lane == 0) counts[(size_t)tile * kWavesPerBlock + wave] = wave_total;
}

// Dense-path layout decided ON THE DEVICE, so that the host does not wait for it: window w gets a direct-address table over
// [first p_id, last p_id] when that range is at least its rows and at most 8 x its rows + 1024 (the host sized the arena for exactly
// that bound).  One window that does not qualify declines the whole call: every range becomes 0 (nothing is built, nothing joins) and
// info[1] = 0 tells the host, at its single synchronisation, to run the general path instead.
// First and last id: two loads per window instead of a pass over the column (segment_stats_kernel: 0.03 ms per 2e7 persons).  For strictly
// increasing ids -- which q3_build_kernel verifies row by row while it builds -- they are the minimum and the maximum.  info[2] = 1
// when some window's range exceeds its rows (gaps: slots no person writes, so the table is filled with -1 first).
__global__ __launch_bounds__(kBlock) void q3_edge_layout_kernel(const int32_t *__restrict__ p_id, const int64_t *__restrict__ seg_off,
                                                                const int32_t *__restrict__ tile_first, int32_t n_win, int32_t bits_mode,
                                                                WinTable *__restrict__ wins, uint64_t *__restrict__ info) {
    __shared__ uint64_t s_wave[kWavesPerBlock];
    __shared__ uint64_t s_carry;
    int ok = 1, gaps = 0;
    for (int32_t w = threadIdx.x; w < n_win; w += kBlock) {
        const int64_t lo = seg_off[2 * w], hi = seg_off[2 * w + 1];
        if (hi <= lo) continue;
        const int64_t range = (int64_t)p_id[hi - 1] - (int64_t)p_id[lo] + 1;
        if (range < hi - lo || range > 8 * (hi - lo) + 1024) ok = 0;
        if (range != hi - lo) gaps = 1;
    }
    ok = __syncthreads_and(ok);
    gaps = __syncthreads_or(gaps);
    const int qualifies = ok;
    if (bits_mode && gaps) ok = 0;   // the bit-block kernels were launched, but some window needs the row table: declined, info[2] says why
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    for (int32_t w0 = 0; w0 < n_win; w0 += kBlock) {
        const int32_t w = w0 + (int32_t)threadIdx.x;
        uint64_t range = 0, entries = 0;
        int32_t base = 0;
        int64_t lo = 0;
        bool gapless = false;
        if (ok && w < n_win && seg_off[2 * w + 1] > seg_off[2 * w]) {
            lo = seg_off[2 * w];
            base = p_id[lo];
            range = (uint64_t)((int64_t)p_id[seg_off[2 * w + 1] - 1] - (int64_t)base + 1);
            gapless = range == (uint64_t)(seg_off[2 * w + 1] - lo);
            entries = bits_mode ? 0 : range;
        }
        const uint64_t incl = wave_incl_scan_u64(entries);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint64_t off = s_carry + incl - entries;
        for (int v = 0; v < wave; ++v) off += s_wave[v];
        if (w < n_win)
            wins[w] = WinTable{base, (uint32_t)range, off, (int32_t)lo, gapless ? tile_first[w] : 0, (uint32_t)(lo - (lo & ~int64_t(3))), gapless ? 1u : 0u};
        __syncthreads();
        if (threadIdx.x == kBlock - 1) s_carry = off + entries;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        info[0] = s_carry;  // entries in use
        info[1] = (uint64_t)ok;
        info[2] = (uint64_t)(qualifies && gaps);   // table mode: fill first; bits mode: declined only because of gaps
    }
}

// RANGE path: every slot of a window's table starts out as kUnwritten and every person stores into the slot of its id -- its row or -1.
// The ids of a window are pairwise different exactly when the slots written are as many as its persons (two persons with one id
// share a slot); a window where they are not voids the call, the hash join (a multimap: duplicate keys join every partner) decides.
constexpr int32_t kUnwritten = (int32_t)0xFEFEFEFE;   // what hipMemset's byte 0xFE leaves; negative like -1: never taken for a row
__global__ __launch_bounds__(kBlock) void q3_table_unique_kernel(const WinTable *__restrict__ wins, const int32_t *__restrict__ direct,
                                                                 const int64_t *__restrict__ seg_off, uint32_t *err) {
    __shared__ uint64_t s_red[kWavesPerBlock];
    const WinTable wt = wins[blockIdx.x];
    uint64_t n = 0;
    for (uint32_t i = threadIdx.x; i < wt.range; i += kBlock) n += direct[wt.off + i] != kUnwritten ? 1u : 0u;
    n = wave_sum_u64(n);
    if (lane_id() == 0) s_red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0 && s_red[0] + s_red[1] + s_red[2] + s_red[3] != (uint64_t)(seg_off[2 * blockIdx.x + 1] - seg_off[2 * blockIdx.x])) atomicOr(err, 1u);
}

// RANGE path, windows whose id range fits LDS (NEXMark's 1-s epochs: 20 000 persons = 80 KB): ONE workgroup per window inverts the
// window's persons -- table[p_id - min] = row where the state filter kept the person (its bit in `bits`, written by the streaming build
// kernel), -1 where it did not -- in LDS and writes the finished table out with coalesced stores.  Scattering the rows straight into the
// global table (q3_build_kernel<dense, table>) costs one 32-byte sector read-modify-write per person once the ids are in no order:
// 0.36 ms per 2e7 persons against 0.09 ms ordered.  The slots that stay unwritten are counted on the way out: as many written slots as
// persons <=> the window's ids are pairwise different (else the call is void and the hash join decides).
constexpr int kInvertBlock = 1024;
constexpr int kInvertMaxRange = 28 * 1024;   // entries: 112 KB of the CU's 160 KB
__global__ __launch_bounds__(kInvertBlock) void q3_invert_window_kernel(const int32_t *__restrict__ p_id, const int64_t *__restrict__ seg_off,
                                                                        const WinTable *__restrict__ wins, const uint32_t *__restrict__ bits,
                                                                        int32_t *__restrict__ direct, uint32_t *err) {
    __shared__ int32_t s_tab[kInvertMaxRange];
    __shared__ uint32_t s_cnt[kInvertBlock / 64];
    const int32_t w = (int32_t)blockIdx.x;
    const WinTable wt = wins[w];
    const int64_t lo = seg_off[2 * w], hi = seg_off[2 * w + 1];
    if (hi <= lo || wt.range == 0) return;
    for (uint32_t i = threadIdx.x; i < wt.range; i += kInvertBlock) s_tab[i] = kUnwritten;
    __syncthreads();
    const uint32_t *wbits = bits + (size_t)wt.first_tile * (kFlagTile / 32);
    for (int64_t r = lo + threadIdx.x; r < hi; r += kInvertBlock) {
        const uint32_t idx = (uint32_t)p_id[r] - (uint32_t)wt.base, rel = wt.lead + (uint32_t)(r - lo);
        const bool hit = (wbits[rel >> 5] >> (rel & 31u)) & 1u;
        if (idx < wt.range) s_tab[idx] = hit ? (int32_t)r : -1;   // (two persons with one id: one slot -- the count below notices)
    }
    __syncthreads();
    uint32_t written = 0;
    for (uint32_t i = threadIdx.x; i < wt.range; i += kInvertBlock) {
        const int32_t v = s_tab[i];
        written += v != kUnwritten ? 1u : 0u;
        direct[wt.off + i] = v;
    }
    written = (uint32_t)wave_sum_u64(written);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = written;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t tot = 0;
        for (int k = 0; k < kInvertBlock / 64; ++k) tot += s_cnt[k];
        if (tot != (uint64_t)(hi - lo)) atomicOr(err, 1u);
    }
}

// direct[0 .. info[0]) = -1 when info[2] says some slot is written by no person; the grid covers the arena's bound, workgroups past
// the entries in use (or all of them, without gaps) leave at once
// ---- GENERAL path, the window's hash table in LDS.  The global build was 1e7 compare-and-swaps on 240 MB of tables that a memset had to
// fill first (0.51 + 0.07 ms per 1e9 events); a window's table is a few thousand live slots -- LDS-sized (the same {key, head row} slots and
// `next[]` chains as the global build: hashtab.hpp).  `cap` <= kLdsBuildCap slots: the host's usual 1.5 slots per person of the largest
// window when that fits, else kLdsBuildCap on the bet that the filter drops enough of them (NEXMark: half) -- a window that does not fit
// raises `err` and the host builds AND probes in global memory with the full capacity.
constexpr int kLdsBuildThreads = 1024;
constexpr uint32_t kLdsBuildCap = 18432;   // 144 KB of the CU's 160
// The hash join of a window where its table is BUILT: one 1024-thread workgroup per window inserts the window's persons that passed the
// state filter into the LDS multimap and then walks the window's auction tiles -- four at a time, a
// 256-thread quarter of the workgroup standing for the tile's workgroup of q3_probe_general_kernel<count> -- probing the table IN LDS:
// the category filter, the first link of every passing row's partner chain into `heads`, the tiles' wave counts.  The table never
// leaves the CU: no 144 KB write-out per window, and none of the ~1.2e7 random 8-byte reads of a global table the count pass made
// (0.17 of its 0.30 ms, at the memory side's random-access rate: DESIGN section 10).  The emit pass reads `heads` and `next[]` as before.
__global__ __launch_bounds__(kLdsBuildThreads) void q3_window_join_lds_kernel(const int32_t *__restrict__ p_id, const int32_t *__restrict__ kept_rows,
                                                                              const int64_t *__restrict__ kept_off, uint32_t cap, int32_t *__restrict__ next,
                                                                              uint32_t *err, const int32_t *__restrict__ seller, const int32_t *__restrict__ category,
                                                                              int64_t n_rows, int64_t category_lit, SegTiles st, uint32_t *__restrict__ counts,
                                                                              uint32_t *__restrict__ heads) {
    __shared__ uint64_t s_tab[kLdsBuildCap];
    const int32_t w = (int32_t)blockIdx.x;
    // the window's persons that passed the state filter: a compact row list a streaming pass wrote (q3_state_flag_kernel -> scan -> emit;
    // with the filter inside this kernel its dependent loads -- offsets, then the state's bytes -- were the workgroup's whole build phase:
    // one workgroup per CU hides no latency)
    const int64_t lo = kept_off[w], hi = kept_off[w + 1];
    for (uint32_t i = threadIdx.x; i < cap; i += kLdsBuildThreads) s_tab[i] = kEmpty64;
    __syncthreads();
    constexpr int kPer = 4;
    bool full = false;
    for (int64_t i0 = lo + threadIdx.x; i0 < hi; i0 += (int64_t)kLdsBuildThreads * kPer) {
        int32_t row[kPer], key[kPer];
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int64_t i = i0 + (int64_t)k * kLdsBuildThreads;
            row[k] = i < hi ? kept_rows[i] : -1;
        }
#pragma unroll
        for (int k = 0; k < kPer; ++k) key[k] = p_id[row[k] < 0 ? 0 : row[k]];
#pragma unroll
        for (int k = 0; k < kPer; ++k)
            if (row[k] >= 0 && !multimap_insert_marked(s_tab, cap, next, key[k], row[k])) full = true;
    }
    if (__syncthreads_or(full)) {   // the window's persons do not fit the LDS table: the host repeats the call on the global tables
        if (threadIdx.x == 0) atomicOr(err, 1u);
        return;
    }
    // ---- probe: quarter q of the workgroup takes tile first + 4 g + q of the window
    const int32_t t_first = st.tile_first[w], t_end = st.tile_first[w + 1];
    const int quarter = threadIdx.x >> 8, lt = threadIdx.x & 255, lwave = lt >> 6, lane = lane_id();
    const int32_t rel0 = lwave * kFlagWaveRows + lane * 4;
    constexpr uint32_t kNoHead = 0xFFFFFFFFu;
    for (int32_t tile = t_first + quarter; tile < t_end; tile += kLdsBuildThreads / kBlock) {
        const TileRange tr = st.tiles[tile];
        uint32_t *tile_heads = heads + (size_t)tile * kFlagTile + rel0;
        const int64_t wbase = tr.tile_begin + rel0;
        uint32_t wave_total = 0;
#pragma unroll 1
        for (int half = 0; half < 2; ++half) {   // four iterations' columns requested together, then probed
            int32_t sv[4][4], cv[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                load4_i32(seller, wbase + (half * 4 + i) * 256, n_rows, sv[i]);
                load4_i32(category, wbase + (half * 4 + i) * 256, n_rows, cv[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t r0 = wbase + (half * 4 + i) * 256;
                // the FIRST probe of the lane's four rows goes out together (four LDS reads in flight instead of a chain of them): at the load
                // factor the host sizes for it settles most rows; what is left walks on row by row
                uint32_t head[4], slot[4];
                uint64_t first[4];
                bool need[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t r = r0 + j;
                    need[j] = r >= tr.lo && r < tr.hi && (int64_t)cv[i][j] == category_lit;
                    slot[j] = slot_of((uint32_t)sv[i][j], cap);
                    first[j] = s_tab[need[j] ? slot[j] : 0u];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    head[j] = kNoHead;
                    if (!need[j]) continue;
                    uint64_t cur = first[j];
                    uint32_t sl = slot[j];
                    for (uint32_t probe = 0, lim = probe_limit(cap); probe < lim; ++probe) {
                        if (cur == kEmpty64) break;
                        if ((int32_t)(cur >> 32) == sv[i][j]) {
                            head[j] = (uint32_t)cur;
                            break;
                        }
                        sl = (sl + 1 == cap) ? 0 : sl + 1;
                        cur = s_tab[sl];
                    }
                }
                *reinterpret_cast<uint4 *>(tile_heads + (half * 4 + i) * 256) = make_uint4(head[0], head[1], head[2], head[3]);
                uint32_t mine = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (head[j] != kNoHead)
                        for (uint32_t c = head[j];; c = (uint32_t)next[c & kChainRow]) {
                            ++mine;
                            if (!(c & kChainMore)) break;
                        }
                wave_total += (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_u32(mine), 63);
            }
        }
        if (lane == 0) counts[(size_t)tile * kWavesPerBlock + lwave] = wave_total;
    }
}

__global__ __launch_bounds__(kBlock) void q3_fill_direct_kernel(int32_t *__restrict__ direct, const uint64_t *__restrict__ info) {
    if (!info[2]) return;
    const uint64_t n = info[0] + 4;
    for (uint64_t i = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * 4; i < n; i += (uint64_t)gridDim.x * kBlock * 4) {
        if (i + 4 <= n) *reinterpret_cast<int4 *>(direct + i) = make_int4(-1, -1, -1, -1);
        else
            for (uint64_t k = i; k < n; ++k) direct[k] = -1;
    }
}

// ---- stage 0 on its own (the exchange filters before it shuffles): row flags of one filter each, flag-tile layout
__global__ __launch_bounds__(kBlock) void q3_category_flag_kernel(const int32_t *__restrict__ category, int64_t n_rows, int64_t category_lit,
                                                                  SegTiles st, uint32_t *__restrict__ flag_words, uint32_t *__restrict__ counts) {
    const int32_t tile = (int32_t)blockIdx.x;
    const TileRange tr = locate_tile(st, tile, kFlagTile);
    int32_t c[kFlagIters][4];
    load_flag_tile(category, n_rows, tr, c);
    const int32_t rel_lo = (int32_t)(tr.lo - tr.tile_begin), rel_hi = (int32_t)(tr.hi - tr.tile_begin), rel0 = flag_rel0();
    uint32_t flags = 0;
#pragma unroll
    for (int it = 0; it < kFlagIters; ++it)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t rel = rel0 + it * 256 + j;
            flags |= ((rel >= rel_lo && rel < rel_hi && (int64_t)c[it][j] == category_lit) ? 1u : 0u) << (it * 4 + j);
        }
    store_flags_and_counts(flags, tile, flag_words, counts);
}
__global__ __launch_bounds__(kBlock) void q3_state_flag_kernel(const int32_t *__restrict__ state_off, const uint8_t *__restrict__ state_data,
                                                               int64_t n_rows, SegTiles st, Utf8Lits lits, uint32_t *__restrict__ flag_words,
                                                               uint32_t *__restrict__ counts) {
    const int32_t tile = (int32_t)blockIdx.x;
    const TileRange tr = locate_tile(st, tile, kFlagTile);
    const int64_t wbase = tr.tile_begin + flag_rel0();
    uint32_t flags = 0;
#pragma unroll
    for (int it = 0; it < kFlagIters; ++it) {
        const int64_t r0 = wbase + it * 256;
        int32_t off[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int64_t r = r0 + j;
            off[j] = state_off[r < 0 ? 0 : (r > n_rows ? n_rows : r)];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t r = r0 + j;
            const bool in = r >= tr.lo && r < tr.hi;
            const uint32_t len = in ? (uint32_t)(off[j + 1] - off[j]) : 0u;
            const uint64_t v = utf8_head8(state_data, len ? off[j] : 0, len > 8 ? 8u : len);
            flags |= ((in && len <= 8 && lits_hit(v, len, lits)) ? 1u : 0u) << (it * 4 + j);
        }
    }
    store_flags_and_counts(flags, tile, flag_words, counts);
}

int make_lits(flockgpu_ctx *ctx, const char *const *state_lits, int n_state_lits, Utf8Lits *lits) {
    if (n_state_lits < 0 || n_state_lits > kMaxLits) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "q3: more than 8 literals");
    *lits = Utf8Lits{};
    lits->n = n_state_lits;
    for (int l = 0; l < n_state_lits; ++l) {
        const size_t len = std::strlen(state_lits[l]);
        if (len > 8) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "q3: Utf8 literal longer than 8 bytes");
        lits->len[l] = (uint32_t)len;
        for (size_t k = 0; k < len; ++k) lits->bytes[l] |= (uint64_t)(uint8_t)state_lits[l][k] << (8 * k);
    }
    return FLOCKGPU_OK;
}

}  // namespace

namespace flockgpu {

int q3_stage0_filters(flockgpu_ctx *ctx, const flockgpu_auction_cols *auction, const flockgpu_windows *auction_win,
                      const flockgpu_person_cols *person, const flockgpu_windows *person_win, int64_t category_lit,
                      const char *const *state_lits, int n_state_lits, Q3Stage0 *out) {
    *out = Q3Stage0{};
    FG_TRY(check_windows(ctx, auction_win, auction->rows, "q3.auction"));
    FG_TRY(check_windows(ctx, person_win, person->rows, "q3.person"));
    if (auction->rows >= (int64_t(1) << 31) || person->rows >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "q3: relations are limited to 2^31 rows per call");
    if (auction->rows > 0 && !auction->category) return fail(ctx, FLOCKGPU_ERR_INVALID, "q3: null category column");
    if (person->rows > 0 && (!person->state.offsets || !person->state.data)) return fail(ctx, FLOCKGPU_ERR_INVALID, "q3: null state column");
    if (reinterpret_cast<uintptr_t>(auction->category) & 15) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "q3: category column must be 16-byte aligned");
    Utf8Lits lits;
    FG_TRY(make_lits(ctx, state_lits, n_state_lits, &lits));
    FG_HIP(ctx, hipSetDevice(ctx->device));
    struct Side {
        const char *name;
        const flockgpu_windows *win;
        int64_t rows;
        SegTiles st;
        uint32_t *flags = nullptr, *counts = nullptr;
        uint64_t *base = nullptr;
        int64_t *d_off = nullptr, *h_off = nullptr;
        int32_t *o_rows = nullptr;
    } sides[2] = {{"xq3.f_auction", auction_win, auction->rows, {}}, {"xq3.f_person", person_win, person->rows, {}}};
    for (Side &sd : sides) {
        const int n_win = sd.win->n_windows;
        std::vector<int64_t> sb((size_t)std::max(n_win, 1)), se(sb.size());
        int64_t covered = 0;
        for (int w = 0; w < n_win; ++w) {
            sb[(size_t)w] = sd.win->pane_row_offsets[sd.win->win_pane_lo[w]];
            se[(size_t)w] = sd.win->pane_row_offsets[sd.win->win_pane_hi[w]];
            covered += se[(size_t)w] - sb[(size_t)w];
        }
        const std::string nm = sd.name;
        FG_TRY(build_seg_tiles(ctx, nm.c_str(), sb.data(), se.data(), n_win, kFlagTile, &sd.st));
        FG_TRY(arena_get_t(ctx, (nm + ".flags").c_str(), (size_t)sd.st.n_tiles * kBlock + 4, &sd.flags));
        FG_TRY(arena_get_t(ctx, (nm + ".counts").c_str(), (size_t)sd.st.n_tiles * kWavesPerBlock + 4, &sd.counts));
        FG_TRY(arena_get_t(ctx, (nm + ".tile_base").c_str(), (size_t)sd.st.n_tiles + 2, &sd.base));
        FG_TRY(arena_get_t(ctx, (nm + ".off").c_str(), (size_t)n_win + 2, &sd.d_off));
        FG_TRY(pinned_get_t(ctx, (nm + ".off").c_str(), (size_t)n_win + 2, &sd.h_off));
        FG_TRY(arena_get_t(ctx, (nm + ".rows").c_str(), (size_t)covered + 4, &sd.o_rows));
    }
    if (sides[0].st.n_tiles > 0) {
        LaunchScope ls(ctx, "q3_category_flag_kernel");
        hipLaunchKernelGGL(q3_category_flag_kernel, dim3((unsigned)sides[0].st.n_tiles), dim3(kBlock), 0, ctx->stream, auction->category, auction->rows,
                           category_lit, sides[0].st, sides[0].flags, sides[0].counts);
    }
    FG_TRY(check_launch(ctx, "q3_category_flag_kernel"));
    if (sides[1].st.n_tiles > 0) {
        LaunchScope ls(ctx, "q3_state_flag_kernel");
        hipLaunchKernelGGL(q3_state_flag_kernel, dim3((unsigned)sides[1].st.n_tiles), dim3(kBlock), 0, ctx->stream, person->state.offsets,
                           person->state.data, person->rows, sides[1].st, lits, sides[1].flags, sides[1].counts);
    }
    FG_TRY(check_launch(ctx, "q3_state_flag_kernel"));
    for (Side &sd : sides) {
        FG_TRY(launch_tile_scan(ctx, sd.counts, sd.st.n_tiles, sd.base, sd.st.tile_first, sd.st.n_seg, sd.d_off));
        FG_TRY(emit_flagged_rows(ctx, sd.st, sd.flags, sd.counts, sd.base, sd.o_rows));
        FG_HIP(ctx, hipMemcpyAsync(sd.h_off, sd.d_off, sizeof(int64_t) * ((size_t)sd.win->n_windows + 1), hipMemcpyDeviceToHost, ctx->stream));
    }
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    out->auction_rows = sides[0].o_rows;
    out->person_rows = sides[1].o_rows;
    out->auction_off.assign(sides[0].h_off, sides[0].h_off + auction_win->n_windows + 1);
    out->person_off.assign(sides[1].h_off, sides[1].h_off + person_win->n_windows + 1);
    if (auction_win->n_windows == 0) out->auction_off.assign(1, 0);
    if (person_win->n_windows == 0) out->person_off.assign(1, 0);
    out->n_auctions = out->auction_off.back();
    out->n_persons = out->person_off.back();
    return FLOCKGPU_OK;
}

}  // namespace flockgpu

extern "C" {

int flockgpu_q3_join(flockgpu_ctx *ctx, const flockgpu_auction_cols *auction, const flockgpu_windows *auction_win,
                     const flockgpu_person_cols *person, const flockgpu_windows *person_win, int64_t category_lit,
                     const char *const *state_lits, int n_state_lits, flockgpu_q3_result *out) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    if (!auction || !person || !out || auction->rows < 0 || person->rows < 0)
        return fail(ctx, FLOCKGPU_ERR_INVALID, "q3: null argument");
    FG_TRY(check_windows(ctx, auction_win, auction->rows, "q3.auction"));
    FG_TRY(check_windows(ctx, person_win, person->rows, "q3.person"));
    if (auction_win->n_windows != person_win->n_windows)
        return fail(ctx, FLOCKGPU_ERR_INVALID, "q3: auction and person schedules differ in window count");
    if (auction->rows >= (int64_t(1) << 31) || person->rows >= (int64_t(1) << 31))
        return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "q3: relations are limited to 2^31 rows per call");
    if (auction->rows > 0 && (!auction->a_id || !auction->seller || !auction->category))
        return fail(ctx, FLOCKGPU_ERR_INVALID, "q3: null auction column");
    if (person->rows > 0 && (!person->p_id || !person->state.offsets || !person->name.offsets || !person->city.offsets))
        return fail(ctx, FLOCKGPU_ERR_INVALID, "q3: null person column");
    if ((reinterpret_cast<uintptr_t>(auction->seller) & 15) || (reinterpret_cast<uintptr_t>(auction->category) & 15) ||
        (reinterpret_cast<uintptr_t>(person->p_id) & 15))
        return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "q3: seller, category and p_id columns must be 16-byte aligned");
    Utf8Lits lits;
    FG_TRY(make_lits(ctx, state_lits, n_state_lits, &lits));
    FG_HIP(ctx, hipSetDevice(ctx->device));
    const int n_win = auction_win->n_windows;

    std::vector<int64_t> ab(n_win), ae(n_win), pb(n_win), pe(n_win);
    int64_t max_person_rows = 0;
    for (int w = 0; w < n_win; ++w) {
        ab[w] = auction_win->pane_row_offsets[auction_win->win_pane_lo[w]];
        ae[w] = auction_win->pane_row_offsets[auction_win->win_pane_hi[w]];
        pb[w] = person_win->pane_row_offsets[person_win->win_pane_lo[w]];
        pe[w] = person_win->pane_row_offsets[person_win->win_pane_hi[w]];
        max_person_rows = std::max(max_person_rows, pe[w] - pb[w]);
    }
    SegTiles st_a, st_p;
    FG_TRY(build_seg_tiles(ctx, "q3.auction", ab.data(), ae.data(), n_win, kFlagTile, &st_a));
    FG_TRY(build_seg_tiles(ctx, "q3.person", pb.data(), pe.data(), n_win, kFlagTile, &st_p));

    // per-window key statistics of the persons: {min, max, sorted} x n_win (exact, on the device)
    int32_t *d_stats = nullptr, *h_stats = nullptr;
    FG_TRY(arena_get_t(ctx, "q3.stats", (size_t)3 * std::max(n_win, 1), &d_stats));
    FG_TRY(pinned_get_t(ctx, "q3.stats", (size_t)3 * std::max(n_win, 1), &h_stats));
    uint32_t *counts = nullptr;
    uint64_t *tile_base = nullptr;
    FG_TRY(arena_get_t(ctx, "q3.counts", (size_t)st_a.n_tiles * kWavesPerBlock + 4, &counts));
    FG_TRY(arena_get_t(ctx, "q3.tile_base", (size_t)st_a.n_tiles + 1, &tile_base));
    int64_t *d_off = nullptr, *h_off = nullptr;
    FG_TRY(arena_get_t(ctx, "q3.seg_out_off", (size_t)n_win + 1, &d_off));
    FG_TRY(pinned_get_t(ctx, "q3.seg_out_off", (size_t)n_win + 2, &h_off));
    uint32_t *d_err = nullptr;
    FG_TRY(arena_get_t(ctx, "q3.err", 4, &d_err));
    std::vector<int64_t> &offs = ctx->host_i64["q3.win_out_offsets"];
    int32_t *o_ar = nullptr, *o_pr = nullptr, *o_aid = nullptr;
    Utf8MultiGather g_text;  // name, city, state of the joined persons: one row list, one length pass, one scan, one emit
    const flockgpu_utf8 text_cols[3] = {person->name, person->city, person->state};
    uint64_t n_pairs = 0;

    // The dense path is SPECULATED: whether the persons qualify (strictly increasing p_id over an affordable range in
    // every window -- what the generator and any id-ordered source produce) is decided by a device pass, the whole
    // pipeline is queued behind it, and the host learns the verdict together with the pair counts and the string byte
    // totals in ONE synchronisation (three before: statistics, pair counts, byte totals; ~60 us each at 1e8 events where
    // the kernels take 90 us).  After a call that did not qualify the statistics are read first, as before.
    // iterations of a person tile per build workgroup: all eight when the tiles alone fill the chip, else two
    const int build_y_shift = st_p.n_tiles >= (int64_t)ctx->num_cus * 4 ? 3 : 1;
    std::vector<int64_t> &regime = ctx->host_i64["q3.dense_regime"];
    // 2: dense, every window gapless last time (bit blocks, no row table) -- also where a ctx starts; 1: dense with the row table;
    // 0: the last call took the general path
    if (regime.empty()) regime.push_back(2);
    // (3: the RANGE path -- ids in any order over an affordable range, the row table laid out from exact statistics)
    bool try_dense = n_win > 0, try_range = false;
    // exact statistics, one more wait: after a call that did not qualify for the speculated paths, and when a speculation is declined
    auto look = [&]() -> int {
        FG_TRY(segment_key_stats(ctx, person->p_id, person->rows, st_p, d_stats, d_stats + n_win, d_stats + 2 * n_win));
        FG_HIP(ctx, hipMemcpyAsync(h_stats, d_stats, sizeof(int32_t) * 3 * n_win, hipMemcpyDeviceToHost, ctx->stream));
        FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        bool ordered = true, affordable = true;
        for (int w = 0; w < n_win; ++w) {
            if (pe[w] == pb[w]) continue;
            const int64_t range = (int64_t)h_stats[n_win + w] - (int64_t)h_stats[w] + 1;
            ordered = ordered && h_stats[2 * n_win + w];
            affordable = affordable && range <= 8 * (pe[w] - pb[w]) + 1024;
        }
        try_dense = ordered && affordable;
        try_range = !ordered && affordable;
        return FLOCKGPU_OK;
    };
    if (try_dense && (regime[0] == 0 || regime[0] == 3)) FG_TRY(look());   // the previous call did not qualify: look before building
    bool bits_mode = regime[0] != 1;
    // ---- the steady-state sequence of the gapless dense path: build (layout inline) -> probe -> emit (self-scan) -> Utf8 lengths ->
    // Utf8 bytes (self-scan), FIVE launches and ONE synchronisation, nothing else on the stream: no memset / copy nodes (flags, window
    // offsets and totals are written by the kernels straight into one pinned block), no scan launches (the emitting workgroups sum the
    // lower tiles' counts themselves), no host wait between the Utf8 lengths and bytes (buffers sized from the previous call's totals).
    // At 1e8 events the call was ~12 kernels + 5 copy nodes of 4-17 us each (0.126 ms for 0.085 ms of kernels).  Anything unusual --
    // first call of a ctx, ids with gaps or out of order, an empty person window, totals beyond the estimates, more tiles than a
    // self-scan should read -- takes (or falls through to) the general sequence below, which also refreshes the estimates.
    std::vector<int64_t> &fast = ctx->host_i64["q3.fast_hint"];   // {rows the take is laid out for, byte capacity x 3, valid}
    if (fast.size() != 5) fast.assign(5, 0);
    bool fast_done = false;
    // (beyond a few thousand tiles the self-scans cost more than the scan launches they replace: 1e9 events, 7324 + 3 x 5860 tiles, ran
    // 0.571 vs 0.530 ms -- and there the launches and waits are a small part of the call anyway)
    constexpr int64_t fast_max_tiles = 2048;
    bool fast_ok = try_dense && bits_mode && fast[4] && st_a.n_tiles > 0 && st_a.n_tiles <= fast_max_tiles && st_p.n_tiles > 0;
    for (int w = 0; w < n_win && fast_ok; ++w)
        if (pe[w] == pb[w] && ae[w] > ab[w]) fast_ok = false;   // (a window without persons leaves its table entry unwritten)
    if (fast_ok) {
        const size_t bound_pairs = (size_t)auction->rows;
        WinTable *d_wins = nullptr;
        uint32_t *bits = nullptr, *flag_words = nullptr;
        uint64_t *d_pairs = nullptr, *h_blk = nullptr;
        FG_TRY(arena_get_t(ctx, "q3.wins", (size_t)n_win, &d_wins));
        FG_TRY(arena_get_t(ctx, "q3.state_bits", (size_t)std::max(st_p.n_tiles, 1) * (kFlagTile / 32) + 4, &bits));
        FG_TRY(arena_get_t(ctx, "q3.flag_words", (size_t)st_a.n_tiles * kBlock, &flag_words));
        FG_TRY(arena_get_t(ctx, "q3.fast_pairs", 2, &d_pairs));
        FG_TRY(pinned_get_t(ctx, "q3.fast", (size_t)n_win + 8, &h_blk));   // [0] flags, [1] pairs, [4 ..] window offsets
        FG_TRY(arena_get_t(ctx, "q3.out_auction_row", bound_pairs + 1, &o_ar));
        FG_TRY(arena_get_t(ctx, "q3.out_person_row", bound_pairs + 1, &o_pr));
        FG_TRY(arena_get_t(ctx, "q3.out_a_id", bound_pairs + 1, &o_aid));
        uint32_t *h_flag = reinterpret_cast<uint32_t *>(h_blk);
        int64_t *h_woff = reinterpret_cast<int64_t *>(h_blk + 4);
        h_blk[0] = 0;   // (the previous call's values were read under its synchronisation)
        h_blk[1] = 0;
        {
            LaunchScope ls(ctx, "q3_build_kernel");
            hipLaunchKernelGGL((q3_build_kernel<true, true, true>), dim3((unsigned)st_p.n_tiles, 8u >> build_y_shift), dim3(kBlock), 0, ctx->stream, person->p_id,
                               person->state.offsets, person->state.data, person->rows, st_p, lits, nullptr, nullptr, bits, nullptr, 0u, nullptr, h_flag,
                               build_y_shift, d_wins);
        }
        FG_TRY(check_launch(ctx, "q3_build_kernel"));
        if (st_a.n_tiles < (int64_t)ctx->num_cus * 6) {   // few tiles: sixteen waves per tile
            LaunchScope ls(ctx, "q3_probe_flag_small_kernel");
            launch_probe_small<true>(ctx, st_a.n_tiles, auction->seller, auction->category, auction->rows, category_lit, st_a, d_wins, nullptr, bits, flag_words, counts);
        } else {
            LaunchScope ls(ctx, "q3_probe_flag_kernel");
            const unsigned grid = (unsigned)std::min<int64_t>(st_a.n_tiles, (int64_t)ctx->num_cus * kStreamBlocksPerCu);
            hipLaunchKernelGGL(q3_probe_flag_kernel<true>, dim3(grid), dim3(kBlock), 0, ctx->stream, auction->seller, auction->category, auction->rows, category_lit,
                               st_a, d_wins, nullptr, bits, flag_words, counts);
        }
        FG_TRY(check_launch(ctx, "q3_probe_flag_kernel"));
        {
            LaunchScope ls(ctx, "q3_emit_dense_kernel");
            hipLaunchKernelGGL(q3_emit_dense_self_kernel, dim3((unsigned)st_a.n_tiles), dim3(kBlock), 0, ctx->stream, auction->seller, auction->a_id, st_a, flag_words,
                               counts, d_wins, o_ar, o_pr, o_aid, d_pairs, h_woff, h_blk);
        }
        FG_TRY(check_launch(ctx, "q3_emit_dense_self_kernel"));
        const int64_t take_rows = std::min<int64_t>((int64_t)bound_pairs, std::max<int64_t>(fast[0], 1));
        Utf8FastGather ft;
        const int rc_take = gather_utf8_multi_fast(ctx, "q3.out_text", text_cols, 3, o_pr, take_rows, d_pairs, &fast[1], &ft);
        if (rc_take != FLOCKGPU_OK && rc_take != FLOCKGPU_ERR_UNSUPPORTED) return rc_take;
        FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (!*h_flag) {   // every window gapless and strictly increasing: what was built stands
            n_pairs = h_blk[1];
            offs.assign((size_t)n_win + 1, 0);
            offs[(size_t)n_win] = (int64_t)n_pairs;
            for (int w = n_win - 1; w >= 0; --w) offs[(size_t)w] = ae[w] > ab[w] ? h_woff[w] : offs[(size_t)w + 1];
            regime[0] = 2;
            flockgpu_utf8 text_out[3];
            int64_t text_bytes[3];
            if (rc_take != FLOCKGPU_OK || *ft.h_over || (int64_t)n_pairs > take_rows) {   // estimates too small: the take once more, exactly
                FG_TRY(gather_utf8_multi_begin(ctx, "q3.out_text", text_cols, 3, o_pr, (int64_t)n_pairs, &g_text, nullptr));
                FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
                FG_TRY(gather_utf8_multi_finish(ctx, g_text, text_out, text_bytes));
            } else {
                for (int c = 0; c < 3; ++c) {
                    text_out[c] = ft.out[c];
                    text_bytes[c] = (int64_t)ft.h_tot[c];
                }
            }
            fast[0] = (int64_t)n_pairs + (int64_t)n_pairs / 8 + 4096;
            for (int c = 0; c < 3; ++c) fast[1 + c] = text_bytes[c] + text_bytes[c] / 8 + 65536;
            out->name = text_out[0];
            out->city = text_out[1];
            out->state = text_out[2];
            out->name_bytes = text_bytes[0];
            out->city_bytes = text_bytes[1];
            out->state_bytes = text_bytes[2];
            out->a_id = o_aid;
            out->auction_row = o_ar;
            out->person_row = o_pr;
            out->win_out_offsets = offs.data();
            out->rows = (int64_t)n_pairs;
            fast_done = true;
        } else {
            fast[4] = 0;   // not this input: the general sequence decides between the row table and the hash join
        }
    }
    if (fast_done) return FLOCKGPU_OK;
    for (bool done = false; try_dense && !done;) {
        const size_t bound_entries = bits_mode ? 8 : (size_t)8 * (size_t)person->rows + (size_t)1024 * n_win + 8;
        const size_t bound_pairs = (size_t)auction->rows;  // one person per key: an auction joins at most one
        WinTable *d_wins = nullptr;
        int32_t *direct = nullptr;
        uint32_t *flag_words = nullptr;
        uint64_t *d_info = nullptr, *h_info = nullptr;
        FG_TRY(arena_get_t(ctx, "q3.wins", (size_t)n_win, &d_wins));
        FG_TRY(arena_get_t(ctx, "q3.direct", bound_entries, &direct));
        uint32_t *bits = nullptr;   // one 1 KiB block per person tile (windows without gaps)
        FG_TRY(arena_get_t(ctx, "q3.state_bits", (size_t)std::max(st_p.n_tiles, 1) * (kFlagTile / 32) + 4, &bits));
        FG_TRY(arena_get_t(ctx, "q3.flag_words", (size_t)st_a.n_tiles * kBlock, &flag_words));
        FG_TRY(arena_get_t(ctx, "q3.layout_info", 4, &d_info));
        FG_TRY(pinned_get_t(ctx, "q3.layout_info", 4, &h_info));
        uint32_t *h_err = nullptr;
        FG_TRY(pinned_get_t(ctx, "q3.err", 4, &h_err));
        FG_HIP(ctx, hipMemsetAsync(d_err, 0, sizeof(uint32_t), ctx->stream));
        FG_TRY(arena_get_t(ctx, "q3.out_auction_row", bound_pairs + 1, &o_ar));
        FG_TRY(arena_get_t(ctx, "q3.out_person_row", bound_pairs + 1, &o_pr));
        FG_TRY(arena_get_t(ctx, "q3.out_a_id", bound_pairs + 1, &o_aid));
        hipLaunchKernelGGL(q3_edge_layout_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, person->p_id, st_p.seg_off, st_p.tile_first, n_win,
                           bits_mode ? 1 : 0, d_wins, d_info);
        FG_TRY(check_launch(ctx, "q3_edge_layout_kernel"));
        // (at most 4096 workgroups walk the entries: a grid over the arena's bound is 156 K workgroups at 2e7 persons, 35 us of
        // dispatch even when every one of them leaves at once)
        if (!bits_mode) {
            hipLaunchKernelGGL(q3_fill_direct_kernel, dim3((unsigned)std::min<int64_t>(div_up((int64_t)bound_entries, kBlock * 4), 4096)), dim3(kBlock), 0,
                               ctx->stream, direct, d_info);
            FG_TRY(check_launch(ctx, "q3_fill_direct_kernel"));
        }
        if (st_p.n_tiles > 0) {
            LaunchScope ls(ctx, "q3_build_kernel");
            hipLaunchKernelGGL((bits_mode ? q3_build_kernel<true, true> : q3_build_kernel<true, false>), dim3((unsigned)st_p.n_tiles, 8u >> build_y_shift), dim3(kBlock), 0, ctx->stream,
                               person->p_id, person->state.offsets, person->state.data, person->rows, st_p, lits, d_wins, direct, bits,
                               nullptr, 0u, nullptr, d_err, build_y_shift, (WinTable *)nullptr);
        }
        FG_TRY(check_launch(ctx, "q3_build_kernel"));
        if (st_a.n_tiles > 0 && st_a.n_tiles < (int64_t)ctx->num_cus * 6) {   // few tiles: sixteen waves per tile
            LaunchScope ls(ctx, "q3_probe_flag_small_kernel");
            if (bits_mode) launch_probe_small<true>(ctx, st_a.n_tiles, auction->seller, auction->category, auction->rows, category_lit, st_a, d_wins, direct, bits, flag_words, counts);
            else launch_probe_small<false>(ctx, st_a.n_tiles, auction->seller, auction->category, auction->rows, category_lit, st_a, d_wins, direct, bits, flag_words, counts);
        } else if (st_a.n_tiles > 0) {
            LaunchScope ls(ctx, "q3_probe_flag_kernel");
            const unsigned grid = (unsigned)std::min<int64_t>(st_a.n_tiles, (int64_t)ctx->num_cus * kStreamBlocksPerCu);
            hipLaunchKernelGGL(bits_mode ? q3_probe_flag_kernel<true> : q3_probe_flag_kernel<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, auction->seller,
                               auction->category, auction->rows, category_lit, st_a, d_wins, direct, bits, flag_words, counts);
        }
        FG_TRY(check_launch(ctx, "q3_probe_flag_kernel"));
        FG_TRY(launch_tile_scan(ctx, counts, st_a.n_tiles, tile_base, st_a.tile_first, st_a.n_seg, d_off));
        if (st_a.n_tiles > 0) {
            LaunchScope ls(ctx, "q3_emit_dense_kernel");
            hipLaunchKernelGGL(bits_mode ? q3_emit_dense_kernel<true> : q3_emit_dense_kernel<false>, dim3((unsigned)st_a.n_tiles), dim3(kBlock), 0, ctx->stream, auction->seller,
                               auction->a_id, st_a, flag_words, counts, tile_base, d_wins, direct, o_ar, o_pr, o_aid);
        }
        FG_TRY(check_launch(ctx, "q3_emit_dense_kernel"));
        const uint64_t *d_pairs = tile_base + st_a.n_tiles;
        // The take of the three Utf8 columns is queued before the host knows the pair count: its grid and its scan cover the previous
        // call's count + 1/8 rather than the bound (one pair per auction: 10x the pairs NEXMark's filters leave -- 27 us of scanning
        // empty tiles at 1e8 events, where the whole call takes 150 us).  A call that turns out larger redoes the take (below).
        std::vector<int64_t> &pairs_hint = ctx->host_i64["q3.pairs_hint"];
        if (pairs_hint.empty()) pairs_hint.push_back(0);
        const int64_t take_rows = pairs_hint[0] > 0 ? std::min<int64_t>((int64_t)bound_pairs, pairs_hint[0]) : (int64_t)bound_pairs;
        FG_TRY(gather_utf8_multi_begin(ctx, "q3.out_text", text_cols, 3, o_pr, take_rows, &g_text, d_pairs));
        FG_HIP(ctx, hipMemcpyAsync(h_off, d_off, sizeof(int64_t) * ((size_t)n_win + 1), hipMemcpyDeviceToHost, ctx->stream));
        FG_HIP(ctx, hipMemcpyAsync(h_info, d_info, sizeof(uint64_t) * 3, hipMemcpyDeviceToHost, ctx->stream));
        FG_HIP(ctx, hipMemcpyAsync(h_err, d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (*h_err) h_info[1] = 0;   // some window's ids are not strictly increasing: what was built is void
        if (h_info[1]) {
            done = true;
            regime[0] = bits_mode ? 2 : 1;
            offs.assign(h_off, h_off + n_win + 1);
            n_pairs = (uint64_t)offs[n_win];
            if ((int64_t)n_pairs > take_rows) {   // more pairs than the take was laid out for: once more, exactly
                FG_TRY(gather_utf8_multi_begin(ctx, "q3.out_text", text_cols, 3, o_pr, (int64_t)n_pairs, &g_text, nullptr));
                FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
            }
            gather_utf8_multi_narrow(&g_text, (int64_t)n_pairs);
            pairs_hint[0] = (int64_t)n_pairs + (int64_t)n_pairs / 8 + 4096;
        } else if (bits_mode && !*h_err && h_info[2]) {
            bits_mode = false;  // the windows qualify but some have gaps in their ids: once more, with the row table
        } else {
            try_dense = false;  // some window's persons are unsorted, duplicated or too sparse: general path below
        }
    }
    if (!try_dense && regime[0] != 0 && regime[0] != 3 && n_win > 0) {   // a speculation was declined: what are the ids like?
        FG_TRY(look());
        try_dense = false;   // (ordered and affordable by the statistics, yet declined: not an input for the dense kernels)
    }
    if (try_range && !try_dense) {
        // ---- the RANGE path (round 4): ids dense in range but in no particular order (several generators interleaved, Kafka partitions, a
        // shuffled replay).  The row table of the dense path needs no order -- only a layout, which exact statistics give, and pairwise
        // different ids, which the table itself shows (q3_table_unique_kernel).  No hash table: with the persons shuffled inside every window
        // the multimap's returning compare-and-swaps cost 0.51 ms per 2e7 persons and its probe ran at 28 % of the HBM rate with 2.7x the
        // algorithmic traffic.
        std::vector<WinTable> h_wins((size_t)n_win);
        uint64_t entries = 0, max_range = 0;
        int32_t tile_at = 0;
        for (int w = 0; w < n_win; ++w) {
            const uint64_t range = pe[w] > pb[w] ? (uint64_t)((int64_t)h_stats[n_win + w] - (int64_t)h_stats[w] + 1) : 0;
            // (first_tile / lead: where the window's rows sit in the row-indexed bit blocks of the streaming build kernel)
            h_wins[(size_t)w] = WinTable{pe[w] > pb[w] ? h_stats[w] : 0, (uint32_t)range, entries, (int32_t)pb[w], tile_at, (uint32_t)(pb[w] - (pb[w] & ~int64_t(3))), 0u};
            entries += range;
            max_range = std::max(max_range, range);
            if (pe[w] > pb[w]) tile_at += (int32_t)div_up(pe[w] - (pb[w] & ~int64_t(3)), kFlagTile);
        }
        const bool invert_in_lds = max_range <= (uint64_t)kInvertMaxRange;   // every window's table fits a workgroup's LDS
        const size_t bound_pairs = (size_t)auction->rows;
        WinTable *d_wins = nullptr, *p_wins = nullptr;
        int32_t *direct = nullptr;
        uint32_t *flag_words = nullptr, *h_err = nullptr;
        FG_TRY(arena_get_t(ctx, "q3.wins", (size_t)n_win, &d_wins));
        FG_TRY(pinned_get_t(ctx, "q3.wins", (size_t)n_win, &p_wins));
        FG_TRY(arena_get_t(ctx, "q3.direct", (size_t)entries + 8, &direct));
        FG_TRY(arena_get_t(ctx, "q3.flag_words", (size_t)st_a.n_tiles * kBlock, &flag_words));
        FG_TRY(pinned_get_t(ctx, "q3.err", 4, &h_err));
        FG_TRY(arena_get_t(ctx, "q3.out_auction_row", bound_pairs + 1, &o_ar));
        FG_TRY(arena_get_t(ctx, "q3.out_person_row", bound_pairs + 1, &o_pr));
        FG_TRY(arena_get_t(ctx, "q3.out_a_id", bound_pairs + 1, &o_aid));
        std::copy(h_wins.begin(), h_wins.end(), p_wins);   // (the staging was last read under the statistics' synchronisation)
        FG_HIP(ctx, hipMemcpyAsync(d_wins, p_wins, sizeof(WinTable) * (size_t)n_win, hipMemcpyHostToDevice, ctx->stream));
        FG_HIP(ctx, hipMemsetAsync(d_err, 0, sizeof(uint32_t), ctx->stream));
        if (st_p.n_tiles > 0 && invert_in_lds) {
            // the state filter as a stream (one bit per person ROW, q3_build_kernel<dense, bits>: no scatter), then one workgroup per window
            // inverts its persons in LDS and writes the finished table with coalesced stores
            uint32_t *bits = nullptr;
            FG_TRY(arena_get_t(ctx, "q3.state_bits", (size_t)std::max(st_p.n_tiles, 1) * (kFlagTile / 32) + 4, &bits));
            {
                LaunchScope ls(ctx, "q3_build_kernel");
                hipLaunchKernelGGL((q3_build_kernel<true, true, false, true>), dim3((unsigned)st_p.n_tiles, 8u >> build_y_shift), dim3(kBlock), 0, ctx->stream, person->p_id,
                                   person->state.offsets, person->state.data, person->rows, st_p, lits, d_wins, nullptr, bits, nullptr, 0u, nullptr, d_err, build_y_shift,
                                   (WinTable *)nullptr);
            }
            FG_TRY(check_launch(ctx, "q3_build_kernel"));
            {
                LaunchScope ls(ctx, "q3_invert_window_kernel");
                hipLaunchKernelGGL(q3_invert_window_kernel, dim3((unsigned)n_win), dim3(kInvertBlock), 0, ctx->stream, person->p_id, st_p.seg_off, d_wins, bits, direct, d_err);
            }
            FG_TRY(check_launch(ctx, "q3_invert_window_kernel"));
        } else if (st_p.n_tiles > 0) {
            FG_HIP(ctx, hipMemsetAsync(direct, 0xFE, sizeof(int32_t) * ((size_t)entries + 4), ctx->stream));
            {
                LaunchScope ls(ctx, "q3_build_kernel");
                hipLaunchKernelGGL((q3_build_kernel<true, false, false, true>), dim3((unsigned)st_p.n_tiles, 8u >> build_y_shift), dim3(kBlock), 0, ctx->stream, person->p_id,
                                   person->state.offsets, person->state.data, person->rows, st_p, lits, d_wins, direct, nullptr, nullptr, 0u, nullptr, d_err, build_y_shift,
                                   (WinTable *)nullptr);
            }
            FG_TRY(check_launch(ctx, "q3_build_kernel"));
            hipLaunchKernelGGL(q3_table_unique_kernel, dim3((unsigned)n_win), dim3(kBlock), 0, ctx->stream, d_wins, direct, st_p.seg_off, d_err);
            FG_TRY(check_launch(ctx, "q3_table_unique_kernel"));
        }
        if (st_a.n_tiles > 0 && st_a.n_tiles < (int64_t)ctx->num_cus * 6) {
            LaunchScope ls(ctx, "q3_probe_flag_small_kernel");
            launch_probe_small<false>(ctx, st_a.n_tiles, auction->seller, auction->category, auction->rows, category_lit, st_a, d_wins, direct, nullptr, flag_words, counts);
        } else if (st_a.n_tiles > 0) {
            LaunchScope ls(ctx, "q3_probe_flag_kernel");
            const unsigned grid = (unsigned)std::min<int64_t>(st_a.n_tiles, (int64_t)ctx->num_cus * kStreamBlocksPerCu);
            hipLaunchKernelGGL(q3_probe_flag_kernel<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, auction->seller, auction->category, auction->rows, category_lit, st_a,
                               d_wins, direct, nullptr, flag_words, counts);
        }
        FG_TRY(check_launch(ctx, "q3_probe_flag_kernel"));
        FG_TRY(launch_tile_scan(ctx, counts, st_a.n_tiles, tile_base, st_a.tile_first, st_a.n_seg, d_off));
        if (st_a.n_tiles > 0) {
            LaunchScope ls(ctx, "q3_emit_dense_kernel");
            hipLaunchKernelGGL(q3_emit_dense_kernel<false>, dim3((unsigned)st_a.n_tiles), dim3(kBlock), 0, ctx->stream, auction->seller, auction->a_id, st_a, flag_words, counts,
                               tile_base, d_wins, direct, o_ar, o_pr, o_aid);
        }
        FG_TRY(check_launch(ctx, "q3_emit_dense_kernel"));
        std::vector<int64_t> &pairs_hint = ctx->host_i64["q3.pairs_hint"];
        if (pairs_hint.empty()) pairs_hint.push_back(0);
        const int64_t take_rows = pairs_hint[0] > 0 ? std::min<int64_t>((int64_t)bound_pairs, pairs_hint[0]) : (int64_t)bound_pairs;
        FG_TRY(gather_utf8_multi_begin(ctx, "q3.out_text", text_cols, 3, o_pr, take_rows, &g_text, tile_base + st_a.n_tiles));
        FG_HIP(ctx, hipMemcpyAsync(h_off, d_off, sizeof(int64_t) * ((size_t)n_win + 1), hipMemcpyDeviceToHost, ctx->stream));
        FG_HIP(ctx, hipMemcpyAsync(h_err, d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (*h_err) {
            try_range = false;   // two persons of a window share an id: every partner joins, which the multimap provides
        } else {
            regime[0] = 3;
            offs.assign(h_off, h_off + n_win + 1);
            n_pairs = (uint64_t)offs[n_win];
            if ((int64_t)n_pairs > take_rows) {
                FG_TRY(gather_utf8_multi_begin(ctx, "q3.out_text", text_cols, 3, o_pr, (int64_t)n_pairs, &g_text, nullptr));
                FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
            }
            gather_utf8_multi_narrow(&g_text, (int64_t)n_pairs);
            pairs_hint[0] = (int64_t)n_pairs + (int64_t)n_pairs / 8 + 4096;
        }
    }
    if (!try_dense && !try_range) {
        regime[0] = 0;
        const uint64_t cap64 = std::max<uint64_t>(64, (uint64_t)max_person_rows * 3 / 2 + 8);
        if (cap64 >= (uint64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "q3: window too large for one table region");
        // build and probe in LDS, one workgroup per window (q3_window_join_lds_kernel), while the tables fit -- or may fit once the state filter has
        // dropped its share; a ctx whose last such bet was lost builds in global memory until its windows shrink
        std::vector<int64_t> &lds_state = ctx->host_i64["q3.lds_build"];   // {rows of the largest window when a bet was lost}
        if (lds_state.empty()) lds_state.push_back(0);
        bool lds_build = n_win > 0 && st_p.n_tiles > 0 && max_person_rows <= 2 * (int64_t)kLdsBuildCap &&
                         (cap64 <= kLdsBuildCap || lds_state[0] == 0 || max_person_rows < lds_state[0]);
        uint32_t cap = 0;
        uint64_t *tables = nullptr;
        int32_t *next = nullptr;
        FG_TRY(arena_get_t(ctx, "q3.next", (size_t)person->rows + 1, &next));
        uint32_t *heads = nullptr;   // per auction row (tile layout): the join partners the count pass found
        FG_TRY(arena_get_t(ctx, "q3.heads", (size_t)std::max(st_a.n_tiles, 1) * kFlagTile, &heads));
        for (;;) {
            cap = lds_build ? (uint32_t)std::min<uint64_t>(cap64, kLdsBuildCap) : (uint32_t)cap64;
            FG_HIP(ctx, hipMemsetAsync(d_err, 0, sizeof(uint32_t), ctx->stream));
            if (lds_build) {
                // the state filter as a streaming pass of its own (flag tiles -> scan -> compact row list with per-window offsets), then build AND
                // count in one kernel, the window's table in LDS from the first insert to the last probe (round 5; round 4 built in LDS,
                // streamed the table out and probed it from global memory)
                uint32_t *p_flags = nullptr, *p_counts = nullptr;
                uint64_t *p_base = nullptr;
                int64_t *p_off = nullptr;
                int32_t *p_rows = nullptr;
                FG_TRY(arena_get_t(ctx, "q3.kept_flags", (size_t)st_p.n_tiles * kBlock + 4, &p_flags));
                FG_TRY(arena_get_t(ctx, "q3.kept_counts", (size_t)st_p.n_tiles * kWavesPerBlock + 4, &p_counts));
                FG_TRY(arena_get_t(ctx, "q3.kept_base", (size_t)st_p.n_tiles + 1, &p_base));
                FG_TRY(arena_get_t(ctx, "q3.kept_off", (size_t)n_win + 2, &p_off));
                FG_TRY(arena_get_t(ctx, "q3.kept_rows", (size_t)person->rows + 4, &p_rows));
                {
                    LaunchScope ls(ctx, "q3_state_flag_kernel");
                    hipLaunchKernelGGL(q3_state_flag_kernel, dim3((unsigned)st_p.n_tiles), dim3(kBlock), 0, ctx->stream, person->state.offsets, person->state.data,
                                       person->rows, st_p, lits, p_flags, p_counts);
                }
                FG_TRY(check_launch(ctx, "q3_state_flag_kernel"));
                FG_TRY(launch_tile_scan(ctx, p_counts, st_p.n_tiles, p_base, st_p.tile_first, st_p.n_seg, p_off));
                FG_TRY(emit_flagged_rows(ctx, st_p, p_flags, p_counts, p_base, p_rows));
                LaunchScope ls(ctx, "q3_window_join_lds_kernel");
                hipLaunchKernelGGL(q3_window_join_lds_kernel, dim3((unsigned)n_win), dim3(kLdsBuildThreads), 0, ctx->stream, person->p_id, p_rows, p_off, cap, next,
                                   d_err, auction->seller, auction->category, auction->rows, category_lit, st_a, counts, heads);
                FG_TRY(check_launch(ctx, "q3_window_join_lds_kernel"));
            } else {
                FG_TRY(arena_get_t(ctx, "q3.tables", (size_t)cap * std::max(n_win, 1), &tables));
                FG_HIP(ctx, hipMemsetAsync(tables, 0xFF, sizeof(uint64_t) * (size_t)cap * n_win, ctx->stream));
                if (st_p.n_tiles > 0) {
                    LaunchScope ls(ctx, "q3_build_kernel");
                    hipLaunchKernelGGL((q3_build_kernel<false, false>), dim3((unsigned)st_p.n_tiles, 8u >> build_y_shift), dim3(kBlock), 0, ctx->stream,
                                       person->p_id, person->state.offsets, person->state.data, person->rows, st_p, lits, nullptr, nullptr, nullptr,
                                       tables, cap, next, d_err, build_y_shift, (WinTable *)nullptr);
                }
                FG_TRY(check_launch(ctx, "q3_build_kernel"));
                if (st_a.n_tiles > 0) {
                    LaunchScope ls(ctx, "q3_probe_count_kernel");
                    hipLaunchKernelGGL(q3_probe_general_kernel<false>, dim3((unsigned)st_a.n_tiles), dim3(kBlock), 0, ctx->stream,
                                       auction->seller, auction->category, auction->a_id, auction->rows, category_lit, st_a, tables, cap,
                                       next, counts, nullptr, nullptr, nullptr, nullptr, heads);
                }
                FG_TRY(check_launch(ctx, "q3_probe_count_kernel"));
            }
            FG_HIP(ctx, hipMemcpyAsync(h_off + n_win + 1, d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            FG_TRY(launch_tile_scan(ctx, counts, st_a.n_tiles, tile_base, st_a.tile_first, st_a.n_seg, d_off));
            FG_HIP(ctx, hipMemcpyAsync(h_off, d_off, sizeof(int64_t) * ((size_t)n_win + 1), hipMemcpyDeviceToHost, ctx->stream));
            FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
            const bool overflow = *reinterpret_cast<uint32_t *>(h_off + n_win + 1) != 0;
            if (overflow && lds_build && cap64 > kLdsBuildCap) {   // the bet was lost: the same sequence with the full-capacity tables in global memory
                lds_state[0] = max_person_rows;
                lds_build = false;
                continue;
            }
            if (overflow) return fail(ctx, FLOCKGPU_ERR_CAPACITY, "q3: build table overflow (cap %u)", cap);
            if (lds_build) lds_state[0] = 0;
            break;
        }
        offs.assign(h_off, h_off + n_win + 1);
        n_pairs = (uint64_t)offs[n_win];
        if (n_pairs >= (uint64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "q3: join output exceeds 2^31 rows");
        FG_TRY(arena_get_t(ctx, "q3.out_auction_row", (size_t)n_pairs + 1, &o_ar));
        FG_TRY(arena_get_t(ctx, "q3.out_person_row", (size_t)n_pairs + 1, &o_pr));
        FG_TRY(arena_get_t(ctx, "q3.out_a_id", (size_t)n_pairs + 1, &o_aid));
        if (st_a.n_tiles > 0 && n_pairs > 0) {
            LaunchScope ls(ctx, "q3_probe_emit_kernel");
            hipLaunchKernelGGL(q3_probe_general_kernel<true>, dim3((unsigned)st_a.n_tiles), dim3(kBlock), 0, ctx->stream,
                               auction->seller, auction->category, auction->a_id, auction->rows, category_lit, st_a, tables, cap,
                               next, counts, tile_base, o_ar, o_pr, o_aid, heads);
        }
        FG_TRY(check_launch(ctx, "q3_probe_emit_kernel"));
        FG_TRY(gather_utf8_multi_begin(ctx, "q3.out_text", text_cols, 3, o_pr, (int64_t)n_pairs, &g_text));
        FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    flockgpu_utf8 text_out[3];
    int64_t text_bytes[3];
    FG_TRY(gather_utf8_multi_finish(ctx, g_text, text_out, text_bytes));
    if (regime[0] == 2) {   // a gapless dense call: the next one of this ctx may take the five-launch sequence with these estimates
        fast[0] = (int64_t)n_pairs + (int64_t)n_pairs / 8 + 4096;
        for (int c = 0; c < 3; ++c) fast[1 + c] = text_bytes[c] + text_bytes[c] / 8 + 65536;
        fast[4] = 1;
    } else {
        fast[4] = 0;
    }
    out->name = text_out[0];
    out->city = text_out[1];
    out->state = text_out[2];
    out->name_bytes = text_bytes[0];
    out->city_bytes = text_bytes[1];
    out->state_bytes = text_bytes[2];
    out->a_id = o_aid;
    out->auction_row = o_ar;
    out->person_row = o_pr;
    out->win_out_offsets = offs.data();
    out->rows = (int64_t)n_pairs;
    return FLOCKGPU_OK;
}

}  // extern "C"
