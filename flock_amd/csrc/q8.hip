// NEXMark q8 for gfx950: per Tumbling(10 s) window
//   (SELECT p_id, name FROM person GROUP BY p_id, name) P  JOIN  (SELECT seller FROM auction GROUP BY seller) A
//   ON p_id = seller  ->  [p_id, name]
// (benchmarks/src/nexmark/query/q8.sql, q8_plan.fmt:1-10, playground/.../nexmark/q8.dag).
//
// HBM-bound integer work, no MFMA.  Every step is count -> scan -> emit or a plain streaming grid (scan.hpp).
//
// stats   : exact [min, max] of p_id per window and whether the window's p_ids are strictly increasing.
// DENSE path (every window strictly increasing = already DISTINCT, key range affordable -- NEXMark ids are dense
// and time-ordered):
//   sellers : DISTINCT seller as a BITMAP over the window's [min p_id, max p_id] (a seller outside that range can
//             never join).  A tile's keys span a few thousand ids, so the workgroup ORs them into an LDS bitmap
//             (the hot seller -- 3/4 of all auctions, event.rs:255-259 -- is collapsed per wave and never reaches
//             LDS) and flushes the non-zero words with fire-and-forget atomicOr: ~1 global atomic per 16 ids.
//   persons : one bit test per person; the 32 row flags of a lane go out as one word (flag tiles, scan.hpp).
// GENERAL path (any window with unsorted / duplicate p_ids, or a sparse key range): DISTINCT seller as a hash set,
//   DISTINCT (p_id, name) by claiming a slot keyed p_id and comparing full keys with the claimant -- both relations grouped by
//   (window, hash bucket) first so that every table lives in LDS ("hash path, partitioned" below); global tables when a bucket does not fit.
// Both paths leave flag words; tile scan -> row list -> take() of p_id and name finish the query.
#include <algorithm>

#include "gather.hpp"
#include "hashtab.hpp"

using namespace flockgpu;

namespace {

struct WinBitmap {
    int32_t base;       // first key of the window's bitmap (multiple of 32 at or below min p_id)
    uint32_t n_bits;    // 0: the window has no persons
    uint64_t word_off;  // offset of the window's words in the bitmap arena
};

constexpr int kBmLdsWords = 1024;  // 32768 ids: the span an LDS-staged tile may cover

// ---- dense path -------------------------------------------------------------------------------------------------
__device__ __forceinline__ void bitmap_or_global(uint32_t *gw, uint32_t bits) {
    // a stale read can only miss bits (bits are never cleared), which costs a redundant atomic, never a lost one
    if ((*gw & bits) != bits) __hip_atomic_fetch_or(gw, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the gapless layout, derived by every workgroup itself (round 4: no layout launch, no zeroing launch) ---------------------------
// A window whose person ids have NO gaps (last - first + 1 = rows: NEXMark's persons, any id-ordered dense source) gets its bitmap at a
// place the HOST knows without looking at the data: words [(lo >> 5) + 2 w, ...) of one arena, lo = the window's first person row -- a
// window of r rows needs at most r / 32 + 2 words whatever its first id is, and the regions of consecutive windows cannot overlap.  So
// the kernels need no layout table: two loads (the window's first and last id) give base and size.  A window with gaps raises a flag in
// pinned host memory (the call is void: the host runs the sequence with the device-side layout pass); that the ids are strictly
// increasing -- which makes first and last the minimum and the maximum and every row DISTINCT -- is verified row by row by the person pass.
struct GaplessWin {
    WinBitmap wb;
    int64_t lo;        // the window's first person row
    int32_t first_id;  // p_id of that row: person p_id sits in row lo + (p_id - first_id)
};
__device__ __forceinline__ GaplessWin gapless_window(const int32_t *__restrict__ p_id, const int64_t *__restrict__ person_seg_off, int32_t w,
                                                     uint32_t *h_flags) {
    GaplessWin g{WinBitmap{0, 0u, 0}, 0, 0};
    const int64_t lo = person_seg_off[2 * w], hi = person_seg_off[2 * w + 1];
    if (hi <= lo) return g;
    const int32_t first = p_id[lo], last = p_id[hi - 1];
    g.lo = lo;
    g.first_id = first;
    if ((int64_t)last - (int64_t)first + 1 != hi - lo) {
        if (threadIdx.x == 0) __hip_atomic_store(h_flags, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return g;
    }
    const int32_t base = first & ~31;
    g.wb = WinBitmap{base, (uint32_t)(last - base + 1), (uint64_t)(lo >> 5) + 2u * (uint64_t)w};
    return g;
}

// kWords: the span of ids (in 32-id words) a tile may stage in LDS.  Ordered sources: a tile's keys span a few thousand ids (1024 words);
// keys in any order (the range path): a tile spans its whole window -- 8192 words = 262144 ids = 32 KB, four workgroups per CU -- so that
// what reaches memory is still one fire-and-forget OR per touched WORD, consecutive words per wave instruction, not one per row.
template <int kWords>
__device__ __forceinline__ void sellers_bitmap_tile(const int32_t *__restrict__ seller, int64_t n_rows, const TileRange &tr, const WinBitmap wb,
                                                    uint32_t *bitmaps, uint32_t *s_bm, uint32_t *s_red, int32_t (&a)[kFlagIters][4]) {
    // (`a`: the tile's keys, requested by the caller BEFORE it looked its window's layout up: the layout is two or three dependent loads,
    // and a workgroup that waits for them before it asks for its 32 KB of keys pays their latency twice -- 57 vs 53 us per 6e7 auctions)
    {
        uint4 *z = reinterpret_cast<uint4 *>(s_bm);
        for (int s = threadIdx.x; s < kWords / 4; s += kBlock) z[s] = make_uint4(0, 0, 0, 0);
    }
    if (wb.n_bits == 0) return;
    const int32_t rel_lo = (int32_t)(tr.lo - tr.tile_begin), rel_hi = (int32_t)(tr.hi - tr.tile_begin);
    const int32_t rel0 = flag_rel0();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    // bit index of every key (-1 = row outside the window or key outside the bitmap)
    uint32_t mn = 0xFFFFFFFFu, mx = 0;
#pragma unroll
    for (int it = 0; it < kFlagIters; ++it)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t rel = rel0 + it * 256 + j;
            const uint32_t idx = (uint32_t)a[it][j] - (uint32_t)wb.base;
            const bool ok = rel >= rel_lo && rel < rel_hi && idx < wb.n_bits && idx < 0x7fffffffu;
            a[it][j] = ok ? (int32_t)idx : -1;
            if (ok) {
                mn = min(mn, idx);
                mx = max(mx, idx);
            }
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    }
    if (lane == 0) {
        s_red[wave] = mn;
        s_red[kWavesPerBlock + wave] = mx;
    }
    __syncthreads();  // also orders the zeroing of s_bm
    mn = min(min(s_red[0], s_red[1]), min(s_red[2], s_red[3]));
    mx = max(max(s_red[4], s_red[5]), max(s_red[6], s_red[7]));
    if (mn == 0xFFFFFFFFu) return;  // no key of the tile can join
    const uint32_t w0 = mn >> 5, n_words = (mx >> 5) - w0 + 1;
    uint32_t *gbm = bitmaps + wb.word_off;
    const bool staged = n_words <= (uint32_t)kWords;  // block-uniform
    int32_t hot = -2;  // wave-uniform: the key most lanes hold right now (3/4 of the auctions name ONE seller)
#pragma unroll
    for (int it = 0; it < kFlagIters; ++it) {
        // Lanes holding the hot key drop it; one lane sets its bit.  48 lanes OR-ing the same LDS word in one
        // instruction serialise, and a candidate taken from lane 0 alone is wrong one time in four -- so the
        // candidate is kept while it still covers >= 16 lanes and otherwise re-elected from two lanes.
        uint64_t m = __ballot(a[it][0] == hot);
        if (__popcll((unsigned long long)m) < 16) {
            const uint64_t live = __ballot(a[it][0] >= 0);
            hot = -2;
            m = 0;
            if (live) {
                const int l1 = __ffsll((unsigned long long)live) - 1;
                const int32_t c1 = __builtin_amdgcn_readlane(a[it][0], l1);
                const uint64_t m1 = __ballot(a[it][0] == c1);
                hot = c1;
                m = m1;
                const uint64_t rest = live & ~m1;
                if (__popcll((unsigned long long)m1) < 16 && rest) {
                    const int l2 = __ffsll((unsigned long long)rest) - 1;
                    const int32_t c2 = __builtin_amdgcn_readlane(a[it][0], l2);
                    const uint64_t m2 = __ballot(a[it][0] == c2);
                    if (__popcll((unsigned long long)m2) > __popcll((unsigned long long)m1)) {
                        hot = c2;
                        m = m2;
                    }
                }
            }
        }
        const int src = m ? __ffsll((unsigned long long)m) - 1 : -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int32_t v = a[it][j];
            if (v == hot && !(lane == src && j == 0)) v = -1;
            if (v < 0) continue;
            const uint32_t idx = (uint32_t)v, bit = 1u << (idx & 31);
            if (staged) {
                uint32_t *w = &s_bm[(idx >> 5) - w0];
                // a set bit stays set: testing first spares the atomic (and its same-word serialisation)
                if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & bit)) atomicOr(w, bit);
            } else {
                bitmap_or_global(gbm + (idx >> 5), bit);
            }
        }
    }
    if (!staged) return;
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < n_words; s += kBlock) {
        const uint32_t bits = s_bm[s];
        if (bits) bitmap_or_global(gbm + w0 + s, bits);
    }
}

__global__ __launch_bounds__(kBlock) void q8_sellers_bitmap_kernel(const int32_t *__restrict__ seller, int64_t n_rows,
                                                                   SegTiles st, const WinBitmap *__restrict__ wins,
                                                                   uint32_t *bitmaps) {
    __shared__ __attribute__((aligned(16))) uint32_t s_bm[kBmLdsWords];
    __shared__ uint32_t s_red[2 * kWavesPerBlock];
    const TileRange tr = locate_tile(st, (int32_t)blockIdx.x, kFlagTile);
    int32_t a[kFlagIters][4];
    load_flag_tile(seller, n_rows, tr, a);
    sellers_bitmap_tile<kBmLdsWords>(seller, n_rows, tr, wins[tr.seg], bitmaps, s_bm, s_red, a);
}
// keys in any order (range path): the wide LDS stage, kept over up to kWideTiles consecutive tiles of ONE window.  A tile of shuffled ids
// touches nearly every word of its window's bitmap (8192 rows over ~6250 words), so a flush per tile was 15e6 word ORs for 2e7 persons
// (0.12 ms); a workgroup that keeps the stage over four tiles of the window flushes a quarter of that.
constexpr int kBmLdsWordsWide = 8192;
constexpr int kWideTiles = 4;
__device__ __forceinline__ void key_bitmap_wide(const int32_t *__restrict__ key, int64_t n_rows, const SegTiles &st, const WinBitmap *__restrict__ wins,
                                                uint32_t *bitmaps, uint32_t *s_bm) {
    const int32_t t0 = (int32_t)blockIdx.x * kWideTiles, t1 = min(t0 + kWideTiles, st.n_tiles);
    int32_t seg = -1;
    WinBitmap wb{0, 0u, 0};
    uint32_t n_words = 0;
    bool staged = false, dirty = false;
    auto flush = [&]() {   // (block-uniform)
        if (staged && dirty) {
            __syncthreads();
            uint32_t *gbm = bitmaps + wb.word_off;
            for (uint32_t s = threadIdx.x; s < n_words; s += kBlock) {
                const uint32_t bits = s_bm[s];
                if (bits) {
                    bitmap_or_global(gbm + s, bits);
                    s_bm[s] = 0;
                }
            }
            __syncthreads();
        }
        dirty = false;
    };
    {
        uint4 *z = reinterpret_cast<uint4 *>(s_bm);
        for (int s = threadIdx.x; s < kBmLdsWordsWide / 4; s += kBlock) z[s] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    for (int32_t t = t0; t < t1; ++t) {
        const TileRange tr = locate_tile(st, t, kFlagTile);
        int32_t a[kFlagIters][4];
        load_flag_tile(key, n_rows, tr, a);
        if (tr.seg != seg) {
            flush();
            seg = tr.seg;
            wb = wins[seg];
            n_words = (wb.n_bits + 31) >> 5;
            staged = n_words <= (uint32_t)kBmLdsWordsWide;
        }
        if (wb.n_bits == 0) continue;
        const int32_t rel_lo = (int32_t)(tr.lo - tr.tile_begin), rel_hi = (int32_t)(tr.hi - tr.tile_begin), rel0 = flag_rel0();
        uint32_t *gbm = bitmaps + wb.word_off;
#pragma unroll
        for (int it = 0; it < kFlagIters; ++it)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int32_t rel = rel0 + it * 256 + j;
                const uint32_t idx = (uint32_t)a[it][j] - (uint32_t)wb.base;
                if (!(rel >= rel_lo && rel < rel_hi && idx < wb.n_bits)) continue;
                const uint32_t bit = 1u << (idx & 31);
                if (staged) {
                    uint32_t *w = &s_bm[idx >> 5];
                    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & bit)) atomicOr(w, bit);
                } else {
                    bitmap_or_global(gbm + (idx >> 5), bit);
                }
            }
        dirty = true;
    }
    flush();
}
__global__ __launch_bounds__(kBlock) void q8_key_bitmap_wide_kernel(const int32_t *__restrict__ key, int64_t n_rows, SegTiles st,
                                                                    const WinBitmap *__restrict__ wins, uint32_t *bitmaps) {
    __shared__ __attribute__((aligned(16))) uint32_t s_bm[kBmLdsWordsWide];
    key_bitmap_wide(key, n_rows, st, wins, bitmaps, s_bm);
}
// (the same pass over the persons' ids -- the presence bitmap of the uniqueness check -- under a name of its own, so that profiles tell
// the two launches apart)
__global__ __launch_bounds__(kBlock) void q8_person_bitmap_wide_kernel(const int32_t *__restrict__ key, int64_t n_rows, SegTiles st,
                                                                       const WinBitmap *__restrict__ wins, uint32_t *bitmaps) {
    __shared__ __attribute__((aligned(16))) uint32_t s_bm[kBmLdsWordsWide];
    key_bitmap_wide(key, n_rows, st, wins, bitmaps, s_bm);
}
// the same with the gapless layout derived in place (the auction tile's window index names the person window)
__global__ __launch_bounds__(kBlock) void q8_sellers_bitmap_inline_kernel(const int32_t *__restrict__ seller, int64_t n_rows, SegTiles st,
                                                                          const int32_t *__restrict__ p_id, const int64_t *__restrict__ person_seg_off,
                                                                          uint32_t *bitmaps, uint32_t *h_flags) {
    __shared__ __attribute__((aligned(16))) uint32_t s_bm[kBmLdsWords];
    __shared__ uint32_t s_red[2 * kWavesPerBlock];
    const TileRange tr = locate_tile(st, (int32_t)blockIdx.x, kFlagTile);
    int32_t a[kFlagIters][4];
    load_flag_tile(seller, n_rows, tr, a);
    const GaplessWin g = gapless_window(p_id, person_seg_off, tr.seg, h_flags);
    sellers_bitmap_tile<kBmLdsWords>(seller, n_rows, tr, g.wb, bitmaps, s_bm, s_red, a);
}

// kOrdered: the layout came from the windows' first and last ids and every row is taken for DISTINCT -- both hold for strictly increasing
// ids, verified here; else (the range path): layout from exact statistics, uniqueness checked by q8_unique_check_kernel, any order.
template <bool kOrdered>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4))) void q8_persons_flag_kernel(const int32_t *__restrict__ p_id, int64_t n_rows,
                                                                 SegTiles st, const WinBitmap *__restrict__ wins,
                                                                 const uint32_t *__restrict__ bitmaps,
                                                                 uint32_t *__restrict__ flag_words,
                                                                 uint32_t *__restrict__ counts, uint32_t *err) {
    int32_t tile = (int32_t)blockIdx.x;
    if (tile >= st.n_tiles) return;
    TileRange tr = locate_tile(st, tile, kFlagTile);
    const int32_t rel0 = flag_rel0();
    const int lane = lane_id();
#pragma unroll 1
    for (;;) {  // tiles b, b + G, ... with the next descriptor requested early (scan.hpp)
        int32_t a[kFlagIters][4];
        load_flag_tile(p_id, n_rows, tr, a);
        // the id in front of each of the wave's eight 256-row chunks (one address per wave; requested with the tile, not under a branch later)
        int32_t before[kFlagIters];
#pragma unroll
        for (int it = 0; it < kFlagIters; ++it) {
            const int64_t r = tr.tile_begin + (rel0 - lane * 4) + it * 256 - 1;
            before[it] = p_id[r < 0 ? 0 : (r < n_rows ? r : n_rows - 1)];   // (clamped into the column: the chunks of a ragged last tile lie past its end)
        }
        const WinBitmap wb = wins[tr.seg];
        const int32_t next = tile + (int32_t)gridDim.x;
        TileRange trn = tr;
        if (next < st.n_tiles) trn = locate_tile(st, next, kFlagTile);
        const int32_t rel_lo = (int32_t)(tr.lo - tr.tile_begin), rel_hi = (int32_t)(tr.hi - tr.tile_begin);
        const uint32_t *gbm = bitmaps + wb.word_off;
        uint32_t flags = 0;
#pragma unroll
        for (int it = 0; it < kFlagIters; ++it)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int32_t rel = rel0 + it * 256 + j;
                const uint32_t idx = (uint32_t)a[it][j] - (uint32_t)wb.base;
                const bool row_in = rel >= rel_lo && rel < rel_hi;
                const bool in = row_in && idx < wb.n_bits;
                // The layout came from the window's first and last id alone (q8_edge_layout_kernel): that they are the minimum and the
                // maximum, and that every row is already DISTINCT, holds when the ids are strictly increasing -- verified here, row against
                // predecessor; a violation voids the call (general path), reported with the results in the same synchronisation.
                if (kOrdered && row_in && wb.n_bits) {
                    int32_t prev;
                    if (j > 0) prev = a[it][j - 1];
                    else {
                        prev = __shfl_up(a[it][3], 1, 64);
                        if (lane == 0) prev = before[it];
                    }
                    if (!(rel == rel_lo || a[it][j] > prev) || idx >= wb.n_bits) atomicOr(err, 1u);
                }
                // unconditional load from a clamped index: loads under per-row branches queue behind each other
                const bool f = in & ((gbm[in ? idx >> 5 : 0u] >> (idx & 31)) & 1u);
                flags |= (f ? 1u : 0u) << (it * 4 + j);
            }
        store_flags_and_counts(flags, tile, flag_words, counts);
        if (next >= st.n_tiles) break;
        tile = next;
        tr = trn;
    }
}

// ---- general path -----------------------------------------------------------------------------------------------
// DISTINCT seller, general keys, staged in LDS: the tile's keys are made distinct in an LDS set first (8192 slots; inserts are LDS
// compare-and-swaps; a key that finds no room within 32 slots goes to the global set directly), and only the distinct ones -- ~700 of 8192 for NEXMark's sellers -- go
// on to the window's set in global memory, where most of them are found present with one load.  (Straight to the global set, row
// by row: 1.09 ms per 6e7 auctions, 18x the bitmap kernel of the dense path; with the loads of a lane's four rows grouped: 1.34 ms.)
constexpr int kLdsSetSlots = 8192;     // 32 KB: four workgroups per CU (16384 slots = two per CU: 0.79 ms instead of 0.64 per 6e7 auctions)
constexpr int kLdsSetMaxProbe = 32;    // a longer run means the tile is full of distinct keys: that key goes straight to the global set
__global__ __launch_bounds__(kBlock) void q8_sellers_set_kernel(const int32_t *__restrict__ seller, int64_t n_rows,
                                                                SegTiles st, uint64_t *sets, uint32_t cap, uint32_t *err) {
    __shared__ uint32_t s_set[kLdsSetSlots];
    __shared__ uint32_t s_has_m1;
    const TileRange tr = locate_tile(st, (int32_t)blockIdx.x, kFlagTile);
    uint64_t *set = sets + (size_t)tr.seg * cap;
    int32_t key[kFlagIters][4];
    load_flag_tile(seller, n_rows, tr, key);
    {
        uint4 *z = reinterpret_cast<uint4 *>(s_set);
        for (int i = threadIdx.x; i < kLdsSetSlots / 4; i += kBlock) z[i] = make_uint4(kEmpty32, kEmpty32, kEmpty32, kEmpty32);
        if (threadIdx.x == 0) s_has_m1 = 0;
    }
    __syncthreads();
    const int32_t rel_lo = (int32_t)(tr.lo - tr.tile_begin), rel_hi = (int32_t)(tr.hi - tr.tile_begin), rel0 = flag_rel0();
    const int lane = lane_id();
#pragma unroll
    for (int it = 0; it < kFlagIters; ++it) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t rel = rel0 + it * 256 + j;
            bool live = rel >= rel_lo && rel < rel_hi;
            const uint32_t k = (uint32_t)key[it][j];
            // the key most lanes hold (3/4 of a window's auctions name one of a few sellers) is inserted by one lane
            const uint32_t hot = __builtin_amdgcn_readfirstlane(k);
            const uint64_t same = __ballot(live && k == hot);
            if (live && k == hot && mbcnt(same) != 0) live = false;
            if (!live) continue;
            if (k == kEmpty32) {   // -1 is the empty mark of the LDS slots: kept aside
                s_has_m1 = 1;
                continue;
            }
            uint32_t sl = (k * kFibHash) >> (32 - 13);
            bool placed = false;
            for (int probe = 0; probe < kLdsSetMaxProbe; ++probe) {
                const uint32_t cur = s_set[sl];
                if (cur == k) { placed = true; break; }
                if (cur == kEmpty32) {
                    const uint32_t old = atomicCAS(&s_set[sl], kEmpty32, k);
                    if (old == kEmpty32 || old == k) { placed = true; break; }
                }
                sl = (sl + 1) & (kLdsSetSlots - 1);
            }
            if (!placed && set_insert(set, cap, (int32_t)k, 0) < 0) atomicOr(err, 1u);
        }
    }
    __syncthreads();
    // The distinct keys sit in ~5 % of the LDS slots.  Walking the slots and inserting where one is occupied leaves ~3 lanes of a wave
    // busy per step, each step as long as one insert's chain of dependent global operations (64 steps per lane: 1.8 ms per 6e7
    // auctions).  So every wave gathers the occupied slots of its share into a queue and inserts 64 keys at a time, all lanes busy.
    __shared__ uint32_t s_q[kWavesPerBlock][128];
    uint32_t *q = s_q[threadIdx.x >> 6];   // this wave's queue (LDS instructions; a volatile pointer compiled to system-scope FLAT accesses)
    uint32_t qn = 0;   // wave-uniform
    auto insert = [&](uint32_t k) {
        const uint64_t first = ld64(&set[slot_of(k, cap)]);
        if (first != kEmpty64 && (uint32_t)(first >> 32) == k) return;   // already in the window's set
        if (set_insert(set, cap, (int32_t)k, 0) < 0) atomicOr(err, 1u);
    };
    for (int i = threadIdx.x; i < kLdsSetSlots; i += kBlock) {
        const uint32_t k = s_set[i];
        const bool occ = k != kEmpty32;
        const uint64_t b = __ballot(occ);
        if (occ) __hip_atomic_store(&q[qn + mbcnt(b)], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        qn += (uint32_t)__popcll((unsigned long long)b);
        __builtin_amdgcn_wave_barrier();
        if (qn >= 64) {
            qn -= 64;
            const uint32_t mine = __hip_atomic_load(&q[qn + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            __builtin_amdgcn_wave_barrier();
            insert(mine);
        }
    }
    if ((uint32_t)lane < qn) insert(__hip_atomic_load(&q[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT));
    if (threadIdx.x == 0 && s_has_m1 && set_insert(set, cap, -1, 0) < 0) atomicOr(err, 1u);
}

__device__ __forceinline__ bool same_person(const int32_t *__restrict__ p_id, const int32_t *__restrict__ name_off,
                                            const uint8_t *__restrict__ name, int64_t a, int64_t b) {
    if (p_id[a] != p_id[b]) return false;
    const int32_t ab = name_off[a], ae = name_off[a + 1], bb = name_off[b], be = name_off[b + 1];
    if (ae - ab != be - bb) return false;
    for (int32_t k = 0; k < ae - ab; ++k)
        if (name[ab + k] != name[bb + k]) return false;
    return true;
}

__global__ __launch_bounds__(kBlock) void q8_persons_general_kernel(const int32_t *__restrict__ p_id, int64_t n_rows,
                                                                    const int32_t *__restrict__ name_off,
                                                                    const uint8_t *__restrict__ name, SegTiles st,
                                                                    uint32_t *ptabs, uint32_t pcap, const uint64_t *sets,
                                                                    uint32_t scap, uint32_t *__restrict__ flag_words,
                                                                    uint32_t *__restrict__ counts, uint32_t *err) {
    const int32_t tile = (int32_t)blockIdx.x;
    const TileRange tr = locate_tile(st, tile, kFlagTile);
    uint32_t *ptab = ptabs + (size_t)tr.seg * pcap;
    const uint64_t *set = sets + (size_t)tr.seg * scap;
    const int64_t wbase = tr.tile_begin + flag_rel0();
    // keys of the whole tile first, then per iteration the first probes of BOTH tables for the lane's four rows together (the seller
    // set is read-only here; the DISTINCT table's first slot is read before it is claimed): one row after the other -- claim, compare,
    // look up -- was four dependent round trips per row, 32 rows per lane (1.40 ms per 2e7 persons)
    int32_t key[kFlagIters][4];
    load_flag_tile(p_id, n_rows, tr, key);
    uint32_t flags = 0;
#pragma unroll 2
    for (int it = 0; it < kFlagIters; ++it) {
        const int64_t r0 = wbase + it * 256;
        bool in[4];
        uint32_t ps[4], ss[4], pfirst[4];
        uint64_t sfirst[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            in[j] = r0 + j >= tr.lo && r0 + j < tr.hi;
            ps[j] = slot_of((uint32_t)key[it][j], pcap);
            ss[j] = slot_of((uint32_t)key[it][j], scap);
            pfirst[j] = __hip_atomic_load(&ptab[in[j] ? ps[j] : 0u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sfirst[j] = set[in[j] ? ss[j] : 0u];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!in[j]) continue;
            const int64_t r = r0 + j;
            const int32_t k = key[it][j];
            // is the person's id a seller of the window at all?  (most are not: no claim, no name compare for them)
            bool sells = false;
            {
                uint64_t cur = sfirst[j];
                uint32_t sl = ss[j];
                for (uint32_t probe = 0, lim = probe_limit(scap); probe < lim; ++probe) {
                    if (cur == kEmpty64) break;
                    if ((int32_t)(cur >> 32) == k) {
                        sells = true;
                        break;
                    }
                    sl = (sl + 1 == scap) ? 0 : sl + 1;
                    cur = set[sl];
                }
            }
            if (!sells) continue;
            // DISTINCT (p_id, name): the first claimant of a slot represents its key
            uint32_t s = ps[j], cur = pfirst[j];
            bool unique = false, done = false;
#pragma unroll 1
            for (uint32_t probe = 0, lim = probe_limit(pcap); probe < lim && !done; ++probe) {
                if (probe) cur = __hip_atomic_load(&ptab[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur == kEmpty32) {
                    uint32_t expected = kEmpty32;
                    if (__hip_atomic_compare_exchange_strong(&ptab[s], &expected, (uint32_t)r, __ATOMIC_RELAXED,
                                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                        unique = true;
                        done = true;
                        break;
                    }
                    cur = expected;
                }
                if (same_person(p_id, name_off, name, r, (int64_t)cur)) {
                    done = true;  // duplicate of an earlier claimant
                    break;
                }
                s = (s + 1 == pcap) ? 0 : s + 1;
            }
            if (!done) atomicOr(err, 1u);
            if (unique) flags |= 1u << (it * 4 + j);
        }
    }
    store_flags_and_counts(flags, tile, flag_words, counts);
}

// ---- hash path, partitioned (round 4) ------------------------------------------------------------------------------------------
// The tables above live in global memory: every distinct seller and every selling person is a RETURNING compare-and-swap on a slot of a
// 240 MB / 120 MB arena (~1e10 of them per second: 0.63 + 1.09 ms per 1e9 events).  Here both relations are first grouped by
// (window, hash bucket) -- per 8192-row tile, in LDS, into the tile's own region of a side buffer: no global cursors, no atomics on global
// memory -- with buckets small enough that one workgroup per (window, bucket) holds the bucket's DISTINCT seller set and its
// {p_id, row} table in LDS.  All compare-and-swaps become LDS instructions; global memory sees streaming reads and writes and one
// fire-and-forget OR per result row.  A bucket that does not fit (skewed hashes, a window of same-id persons with different names)
// raises `err`: the host repeats the call on the global tables.
constexpr int kPartMaxLog2 = 10;         // up to 1024 buckets per window
constexpr int kPartMaxBuckets = 1 << kPartMaxLog2;
constexpr int kJoinSlotsLog2 = 10, kJoinSlots = 1 << kJoinSlotsLog2;   // LDS slots of a bucket's table of FURTHER names under an id that already has a person (8 KB)
constexpr int kJoinSellLog2 = 12, kJoinSellLog2Large = 14;   // LDS slots of a bucket's seller set {key, first person}: 4096 (32 KB: three
                                                             // workgroups per CU), or 16384 (128 KB: one) once a call of the ctx has
                                                             // overflowed the small one
constexpr int kJoinProbes = 128;
constexpr uint32_t kPartErrSellers = 1u, kPartErrPersons = 2u;
constexpr int kJoinBlock = 512;          // threads of a (window, bucket) workgroup: three of them per CU
constexpr int kJoinWaves = kJoinBlock / 64;
// what the host sizes the bucket count for (averages of the largest window): the person table is then at most ~40 % full; the seller
// set holds DISTINCT sellers, of which NEXMark has ~700 per 8192 auctions -- a window whose auctions all name different sellers needs the
// large set
constexpr int64_t kPartPersonsPerBucket = 1600, kPartAuctionsPerBucket = 6144;

__device__ __forceinline__ uint32_t part_bucket(uint32_t k, int log2nb) { return log2nb ? (k * kFibHash) >> (32 - log2nb) : 0u; }
__device__ __forceinline__ uint32_t part_slot(uint32_t k, int log2nb, int log2slots) {   // the hash bits below the bucket's
    return ((k * kFibHash) >> (32 - log2nb - log2slots)) & ((1u << log2slots) - 1u);
}

// s_cnt[0 .. nb) -> its exclusive prefix, in place (nb <= 4 * kBlock); returns the total.  Ends with a barrier.
__device__ __forceinline__ uint32_t block_excl_scan_lds(uint32_t *s_cnt, int nb, uint32_t *s_red) {
    const int t = (int)threadIdx.x;
    uint32_t v[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = t * 4 + j < nb ? s_cnt[t * 4 + j] : 0u;
        sum += v[j];
    }
    const uint32_t incl = wave_incl_scan_u32(sum);
    if (lane_id() == 63) s_red[t >> 6] = incl;
    __syncthreads();
    uint32_t base = incl - sum;
    for (int w = 0; w < (t >> 6); ++w) base += s_red[w];
    const uint32_t total = s_red[0] + s_red[1] + s_red[2] + s_red[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (t * 4 + j < nb) s_cnt[t * 4 + j] = base;
        base += v[j];
    }
    __syncthreads();
    return total;
}

// A tile's grouped list leaves LDS as 16-byte stores into the tile's region (8192 entries; what lies behind `total` is never read).
__device__ __forceinline__ void part_copy_out_u32(const uint32_t *s_k, uint32_t total, uint32_t *dst) {
    const uint4 *src4 = reinterpret_cast<const uint4 *>(s_k);
    uint4 *dst4 = reinterpret_cast<uint4 *>(dst);
    for (uint32_t i = threadIdx.x; i < (total + 3) / 4; i += kBlock) dst4[i] = src4[i];
}

// Sellers of one tile: DISTINCT in an LDS set first (as q8_sellers_set_kernel; a key that finds no room there is listed as it is -- the
// bucket's set takes duplicates), the distinct keys grouped by bucket: skeys[tile * 8192 + soff[tile][b] .. soff[tile][b + 1]).  The lane
// whose compare-and-swap put a key into the set is the one that lists it: it takes the key's rank in its bucket right then, so the set is
// never walked.  A wave's LDS round trips are what this pass costs (nearly every step has SOME lane with a new key): the four rows of a
// lane's load are probed, claimed and ranked side by side.
__global__ __launch_bounds__(kBlock) void q8_sellers_part_kernel(const int32_t *__restrict__ seller, int64_t n_rows, SegTiles st, int log2nb,
                                                                 uint32_t *__restrict__ skeys, uint16_t *__restrict__ soff) {
    __shared__ __attribute__((aligned(16))) uint32_t s_set[kLdsSetSlots];   // the tile's set; later the grouped list
    __shared__ uint32_t s_cnt[kPartMaxBuckets];
    __shared__ uint32_t s_red[kWavesPerBlock];
    __shared__ uint32_t s_has_m1;
    const int32_t tile = (int32_t)blockIdx.x;
    const TileRange tr = locate_tile(st, tile, kFlagTile);
    const int nb = 1 << log2nb;
    int32_t key[kFlagIters][4];
    load_flag_tile(seller, n_rows, tr, key);
    {
        uint4 *z = reinterpret_cast<uint4 *>(s_set);
        for (int i = threadIdx.x; i < kLdsSetSlots / 4; i += kBlock) z[i] = make_uint4(kEmpty32, kEmpty32, kEmpty32, kEmpty32);
        for (int i = threadIdx.x; i < nb; i += kBlock) s_cnt[i] = 0;
        if (threadIdx.x == 0) s_has_m1 = 0;
    }
    __syncthreads();
    const int32_t rel_lo = (int32_t)(tr.lo - tr.tile_begin), rel_hi = (int32_t)(tr.hi - tr.tile_begin), rel0 = flag_rel0();
    uint32_t listed = 0;   // rows whose key this lane lists: it put the key into the set, or the key found no room there
    uint16_t rank[kFlagIters][4];
#pragma unroll
    for (int it = 0; it < kFlagIters; ++it) {
        bool live[4];
        uint32_t first[4], old[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t rel = rel0 + it * 256 + j;
            live[j] = rel >= rel_lo && rel < rel_hi;
            const uint32_t k = (uint32_t)key[it][j];
            // the key most lanes hold (3/4 of a window's auctions name one of a few sellers) is inserted by one lane
            const uint32_t hot = __builtin_amdgcn_readfirstlane(k);
            const uint64_t same = __ballot(live[j] && k == hot);
            if (live[j] && k == hot && mbcnt(same) != 0) live[j] = false;
            if (live[j] && k == kEmpty32) {   // -1 is the empty mark of the LDS slots: kept aside
                s_has_m1 = 1;
                live[j] = false;
            }
            first[j] = s_set[live[j] ? (k * kFibHash) >> (32 - 13) : 0u];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t k = (uint32_t)key[it][j];
            old[j] = first[j];
            if (live[j] && first[j] == kEmpty32) old[j] = atomicCAS(&s_set[(k * kFibHash) >> (32 - 13)], kEmpty32, k);
        }
        bool mine[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t k = (uint32_t)key[it][j];
            mine[j] = false;
            rank[it][j] = 0;
            if (!live[j]) continue;
            bool won = first[j] == kEmpty32 && old[j] == kEmpty32, placed = won || old[j] == k;
            if (!placed) {   // the home slot holds another key: on from the next one
                uint32_t sl = (((k * kFibHash) >> (32 - 13)) + 1) & (kLdsSetSlots - 1);
                for (int probe = 1; probe < kLdsSetMaxProbe; ++probe) {
                    const uint32_t cur = s_set[sl];
                    if (cur == k) { placed = true; break; }
                    if (cur == kEmpty32) {
                        const uint32_t o = atomicCAS(&s_set[sl], kEmpty32, k);
                        if (o == kEmpty32) { placed = won = true; break; }
                        if (o == k) { placed = true; break; }
                    }
                    sl = (sl + 1) & (kLdsSetSlots - 1);
                }
            }
            mine[j] = won || !placed;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (mine[j]) {
                listed |= 1u << (it * 4 + j);
                rank[it][j] = (uint16_t)atomicAdd(&s_cnt[part_bucket((uint32_t)key[it][j], log2nb)], 1u);
            }
    }
    __syncthreads();
    uint32_t rank_m1 = 0;
    if (threadIdx.x == 0 && s_has_m1) rank_m1 = atomicAdd(&s_cnt[part_bucket(kEmpty32, log2nb)], 1u);
    __syncthreads();
    const uint32_t total = block_excl_scan_lds(s_cnt, nb, s_red);   // (everyone is done with the set: its memory takes the grouped list)
    uint16_t *off = soff + (size_t)tile * (size_t)(nb + 1);
    for (int i = threadIdx.x; i < nb; i += kBlock) off[i] = (uint16_t)s_cnt[i];
    if (threadIdx.x == 0) off[nb] = (uint16_t)total;
    if (listed) {
#pragma unroll
        for (int it = 0; it < kFlagIters; ++it)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (listed & (1u << (it * 4 + j))) s_set[s_cnt[part_bucket((uint32_t)key[it][j], log2nb)] + rank[it][j]] = (uint32_t)key[it][j];
    }
    if (threadIdx.x == 0 && s_has_m1) s_set[s_cnt[part_bucket(kEmpty32, log2nb)] + rank_m1] = kEmpty32;
    __syncthreads();
    part_copy_out_u32(s_set, total, skeys + (size_t)tile * kFlagTile);
}

// Persons of one tile grouped by bucket: {p_id, row within the tile} at pkeys / prel[tile * 8192 + poff[tile][b] ..).  Also zeroes the
// tile's flag BYTES, one per row (the bucket workgroups set the result rows': plain stores -- 1e7 agent-scope ORs into flag words cost
// 0.12 ms per 1e9 events; the bytes are packed into flag words by q8_flag_pack_kernel).
__global__ __launch_bounds__(kBlock) void q8_persons_part_kernel(const int32_t *__restrict__ p_id, int64_t n_rows, SegTiles st, int log2nb,
                                                                 uint32_t *__restrict__ pkeys, uint16_t *__restrict__ prel,
                                                                 uint16_t *__restrict__ poff, uint8_t *__restrict__ flag_bytes) {
    __shared__ __attribute__((aligned(16))) uint32_t s_k[kFlagTile];
    __shared__ __attribute__((aligned(16))) uint16_t s_r[kFlagTile];
    __shared__ uint32_t s_cnt[kPartMaxBuckets];
    __shared__ uint32_t s_red[kWavesPerBlock];
    const int32_t tile = (int32_t)blockIdx.x;
    const TileRange tr = locate_tile(st, tile, kFlagTile);
    const int nb = 1 << log2nb;
    int32_t key[kFlagIters][4];
    load_flag_tile(p_id, n_rows, tr, key);
    for (int i = threadIdx.x; i < nb; i += kBlock) s_cnt[i] = 0;
    {
        uint4 *z = reinterpret_cast<uint4 *>(flag_bytes + (size_t)tile * kFlagTile);
        z[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
        z[threadIdx.x + kBlock] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    const int32_t rel_lo = (int32_t)(tr.lo - tr.tile_begin), rel_hi = (int32_t)(tr.hi - tr.tile_begin), rel0 = flag_rel0();
    uint16_t rank[kFlagIters][4];
#pragma unroll
    for (int it = 0; it < kFlagIters; ++it)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t rel = rel0 + it * 256 + j;
            rank[it][j] = 0;
            if (rel >= rel_lo && rel < rel_hi) rank[it][j] = (uint16_t)atomicAdd(&s_cnt[part_bucket((uint32_t)key[it][j], log2nb)], 1u);
        }
    __syncthreads();
    const uint32_t total = block_excl_scan_lds(s_cnt, nb, s_red);
    uint16_t *off = poff + (size_t)tile * (size_t)(nb + 1);
    for (int i = threadIdx.x; i < nb; i += kBlock) off[i] = (uint16_t)s_cnt[i];
    if (threadIdx.x == 0) off[nb] = (uint16_t)total;
#pragma unroll
    for (int it = 0; it < kFlagIters; ++it)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t rel = rel0 + it * 256 + j;
            if (rel >= rel_lo && rel < rel_hi) {
                const uint32_t pos = s_cnt[part_bucket((uint32_t)key[it][j], log2nb)] + rank[it][j];
                s_k[pos] = (uint32_t)key[it][j];
                s_r[pos] = (uint16_t)rel;
            }
        }
    __syncthreads();
    part_copy_out_u32(s_k, total, pkeys + (size_t)tile * kFlagTile);
    {
        const uint4 *src4 = reinterpret_cast<const uint4 *>(s_r);
        uint4 *dst4 = reinterpret_cast<uint4 *>(prel + (size_t)tile * kFlagTile);
        for (uint32_t i = threadIdx.x; i < (total + 7) / 8; i += kBlock) dst4[i] = src4[i];
    }
}

// The runs of bucket `b` in up to kJoinChunk consecutive tiles [t0, t1) as ONE index space: pref = exclusive prefix of the run lengths
// (pref[n .. kJoinChunk] = the total), o0 = where each run begins in its tile's region.  Loading a chunk's offsets and publishing them are
// two steps, so that both relations' offsets travel together.
constexpr int kJoinChunk = 256;   // tiles of one relation a workgroup indexes at a time
constexpr int kJoinPre = 4;       // person entries per thread requested BEFORE the sellers are inserted (4 x 512: an average bucket whole)
struct PartRun {
    uint32_t len, o0;
};
__device__ __forceinline__ PartRun part_run_load(const uint16_t *__restrict__ offs, int nb, int b, int32_t t0, int32_t n) {
    PartRun r{0u, 0u};
    if ((int32_t)threadIdx.x < n) {
        const uint16_t *o = offs + (size_t)(t0 + (int32_t)threadIdx.x) * (size_t)(nb + 1) + b;
        r.o0 = o[0];
        r.len = (uint32_t)o[1] - r.o0;
    }
    return r;
}
// Returns the entries of the chunk; ends with a barrier.
__device__ __forceinline__ uint32_t part_run_publish(const PartRun &r, uint32_t *pref, uint16_t *o0, uint32_t *s_red) {
    const uint32_t incl = wave_incl_scan_u32(r.len);
    if (lane_id() == 63) s_red[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kJoinWaves; ++w) {
        if (w < (int)(threadIdx.x >> 6)) base += s_red[w];
        total += s_red[w];
    }
    if (threadIdx.x < kJoinChunk) {
        pref[threadIdx.x] = base + incl - r.len;
        o0[threadIdx.x] = (uint16_t)r.o0;
    }
    if (threadIdx.x == 0) pref[kJoinChunk] = total;
    __syncthreads();
    return total;
}
// entry e of the chunk -> the run it lies in (the last i < n with pref[i] <= e: a run of no entries is never chosen)
__device__ __forceinline__ int part_find_run(const uint32_t *pref, int n, uint32_t e) {
    int lo = 0, hi = n;   // pref[lo] <= e < pref[hi]
    while (hi - lo > 1) {   // (the same trips for every lane)
        const int mid = (lo + hi) >> 1;
        if (pref[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// One workgroup per (window, bucket): the bucket's distinct sellers into an LDS set, then every person of the bucket -- is its id in
// the set?  then DISTINCT (p_id, name) by claiming a slot of the LDS table keyed p_id (names compared with the claimant's in global
// memory: only for persons that share an id) -- and the first claimant's row flag is set.  A workgroup's life is a chain of memory
// round trips, so both relations' offsets are requested first and together, and the persons' keys and rows are on their way while the
// sellers are inserted.
__global__ __launch_bounds__(kJoinBlock) void q8_bucket_join_kernel(const int32_t *__restrict__ p_id, const int32_t *__restrict__ name_off,
                                                                    const uint8_t *__restrict__ name, SegTiles st_a, SegTiles st_p, int log2nb,
                                                                    const uint32_t *__restrict__ skeys, const uint16_t *__restrict__ soff,
                                                                    const uint32_t *__restrict__ pkeys, const uint16_t *__restrict__ prel,
                                                                    const uint16_t *__restrict__ poff, uint8_t *__restrict__ flag_bytes,
                                                                    int log2sell, uint32_t *err) {
    extern __shared__ uint32_t s_sell[];   // 1 << log2sell keys, then as many + 1 rows: the first person seen under the key (the last: under -1)
    __shared__ uint64_t s_pers[kJoinSlots];
    __shared__ uint32_t ss_pref[kJoinChunk + 1], sp_pref[kJoinChunk + 1], sp_tbeg[kJoinChunk];
    __shared__ uint16_t ss_o0[kJoinChunk], sp_o0[kJoinChunk];
    __shared__ uint32_t s_red[kJoinWaves];
    __shared__ uint32_t s_m1;
    const int nb = 1 << log2nb;
    const int32_t w = (int32_t)(blockIdx.x >> log2nb), b = (int32_t)(blockIdx.x & (uint32_t)(nb - 1));
    const int32_t ta0 = st_a.tile_first[w], ta1 = st_a.tile_first[w + 1], tp0 = st_p.tile_first[w], tp1 = st_p.tile_first[w + 1];
    if (ta0 == ta1 || tp0 == tp1) return;   // no auctions: nobody sells; no persons: nothing to flag (the flag words are zero)
    const int32_t na0 = ta1 - ta0 < kJoinChunk ? ta1 - ta0 : kJoinChunk, np0 = tp1 - tp0 < kJoinChunk ? tp1 - tp0 : kJoinChunk;
    const PartRun rs0 = part_run_load(soff, nb, b, ta0, na0);
    const PartRun rp0 = part_run_load(poff, nb, b, tp0, np0);
    if ((int32_t)threadIdx.x < np0) sp_tbeg[threadIdx.x] = (uint32_t)st_p.tiles[tp0 + (int32_t)threadIdx.x].tile_begin;   // (rows < 2^31)
    const uint32_t sell_mask = (1u << log2sell) - 1u;
    uint32_t *s_own = s_sell + (1 << log2sell);
    for (int i = threadIdx.x; i < (2 << log2sell) + 1; i += kJoinBlock) s_sell[i] = kEmpty32;
    for (int i = threadIdx.x; i < kJoinSlots; i += kJoinBlock) s_pers[i] = kEmpty64;
    if (threadIdx.x == 0) s_m1 = 0;
    const uint32_t tot_s0 = part_run_publish(rs0, ss_pref, ss_o0, s_red);   // (the barriers also cover the tables' initialisation)
    const uint32_t tot_p0 = part_run_publish(rp0, sp_pref, sp_o0, s_red);
    uint32_t pk[kJoinPre], pr[kJoinPre], pt[kJoinPre];   // key, row within the tile | index of the tile in the chunk << 16
#pragma unroll
    for (int j = 0; j < kJoinPre; ++j) {
        const uint32_t e = threadIdx.x + j * kJoinBlock;
        pk[j] = pr[j] = pt[j] = 0;
        if (e < tot_p0) {
            const int i = part_find_run(sp_pref, np0, e);
            const uint64_t at = (uint64_t)(tp0 + i) * kFlagTile + sp_o0[i] + (e - sp_pref[i]);
            pk[j] = pkeys[at];
            pr[j] = prel[at];
            pt[j] = (uint32_t)i;
        }
    }
    uint32_t bad = 0;
    for (int32_t c0 = ta0; c0 < ta1; c0 += kJoinChunk) {
        const int32_t n = ta1 - c0 < kJoinChunk ? ta1 - c0 : kJoinChunk;
        uint32_t total = tot_s0;
        if (c0 != ta0) {
            __syncthreads();   // (everyone is done with the previous chunk's index)
            total = part_run_publish(part_run_load(soff, nb, b, c0, n), ss_pref, ss_o0, s_red);
        }
        for (uint32_t e0 = threadIdx.x; e0 < total; e0 += kJoinPre * kJoinBlock) {   // kJoinPre keys requested together, then inserted
            uint32_t sk[kJoinPre];
#pragma unroll
            for (int j = 0; j < kJoinPre; ++j) {
                const uint32_t e = e0 + j * kJoinBlock;
                sk[j] = kEmpty32;
                if (e < total) {
                    const int i = part_find_run(ss_pref, n, e);
                    sk[j] = skeys[(uint64_t)(c0 + i) * kFlagTile + ss_o0[i] + (e - ss_pref[i])];
                    if (sk[j] == kEmpty32) s_m1 = 1;
                }
            }
#pragma unroll
            for (int j = 0; j < kJoinPre; ++j) {
                const uint32_t k = sk[j];
                if (k == kEmpty32) continue;
                uint32_t sl = part_slot(k, log2nb, log2sell);
                bool placed = false;
                for (int probe = 0; probe < kJoinProbes; ++probe) {
                    const uint32_t cur = s_sell[sl];
                    if (cur == k) { placed = true; break; }
                    if (cur == kEmpty32) {
                        const uint32_t old = atomicCAS(&s_sell[sl], kEmpty32, k);
                        if (old == kEmpty32 || old == k) { placed = true; break; }
                    }
                    sl = (sl + 1) & sell_mask;
                }
                if (!placed) bad |= kPartErrSellers;
            }
        }
    }
    __syncthreads();   // the set is complete
    // The slot of the id in the set, or -1.  `first` = what the key's home slot held (read by the caller, several persons' at once).
    auto seller_slot = [&](uint32_t k, uint32_t first) -> int32_t {
        if (k == kEmpty32) return s_m1 ? (int32_t)(1 << log2sell) : -1;
        uint32_t sl = part_slot(k, log2nb, log2sell), cur = first;
        for (int probe = 0; probe < kJoinProbes; ++probe) {
            if (cur == k) return (int32_t)sl;
            if (cur == kEmpty32) return -1;
            sl = (sl + 1) & sell_mask;
            cur = s_sell[sl];
        }
        return -1;   // (a run this long has raised the sellers' error bit when it was built)
    };
    // DISTINCT (p_id, name) of a person that sells.  The FIRST person seen under an id owns the id's slot of the set (one compare-and-swap
    // at a slot that is already known: nothing to probe) -- `owner` = what that compare-and-swap returned.  Another person under the same
    // id is compared with the owner's name; a different name goes through the small table of further names.
    auto settle = [&](uint32_t k, uint32_t rel, int32_t tile, uint32_t row, uint32_t owner) {
        bool unique = owner == kEmpty32;
        if (!unique && !same_person(p_id, name_off, name, (int64_t)row, (int64_t)owner)) {
            const uint64_t mine = ((uint64_t)k << 32) | row;
            uint32_t sl = part_slot(k, log2nb, kJoinSlotsLog2);
            bool done = false;
#pragma unroll 1
            for (int probe = 0; probe < kJoinProbes; ++probe) {
                uint64_t cur = __hip_atomic_load(&s_pers[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (cur == kEmpty64) {
                    cur = atomicCAS(reinterpret_cast<unsigned long long *>(&s_pers[sl]), (unsigned long long)kEmpty64, (unsigned long long)mine);
                    if (cur == kEmpty64) {
                        unique = done = true;
                        break;
                    }
                }
                if ((uint32_t)(cur >> 32) == k && same_person(p_id, name_off, name, (int64_t)row, (int64_t)(uint32_t)cur)) {
                    done = true;   // duplicate of an earlier claimant
                    break;
                }
                sl = (sl + 1) & (uint32_t)(kJoinSlots - 1);
            }
            if (!done) bad |= kPartErrPersons;
        }
        if (unique) flag_bytes[(size_t)tile * kFlagTile + rel] = 1;
    };
    {   // the requested entries: every stage for all of them together (LDS round trips in flight side by side)
        int32_t slot[kJoinPre];
        uint32_t first[kJoinPre], owner[kJoinPre];
#pragma unroll
        for (int j = 0; j < kJoinPre; ++j) {
            slot[j] = threadIdx.x + j * kJoinBlock < tot_p0 ? 0 : -1;
            first[j] = s_sell[slot[j] == 0 && pk[j] != kEmpty32 ? part_slot(pk[j], log2nb, log2sell) : 0u];
        }
#pragma unroll
        for (int j = 0; j < kJoinPre; ++j)
            if (slot[j] == 0) slot[j] = seller_slot(pk[j], first[j]);
#pragma unroll
        for (int j = 0; j < kJoinPre; ++j) owner[j] = slot[j] >= 0 ? atomicCAS(&s_own[slot[j]], kEmpty32, sp_tbeg[pt[j]] + pr[j]) : 0u;
#pragma unroll
        for (int j = 0; j < kJoinPre; ++j)
            if (slot[j] >= 0) settle(pk[j], pr[j], tp0 + (int32_t)pt[j], sp_tbeg[pt[j]] + pr[j], owner[j]);
    }
    // what the bucket holds beyond the requested entries (a bucket far above the average).  A window's person tiles fit ONE chunk: the
    // host takes this path only then (at most 1600 x 1024 persons per window: 200 tiles).
    for (uint32_t e = threadIdx.x + kJoinPre * kJoinBlock; e < tot_p0; e += kJoinBlock) {
        const int i = part_find_run(sp_pref, np0, e);
        const uint64_t at = (uint64_t)(tp0 + i) * kFlagTile + sp_o0[i] + (e - sp_pref[i]);
        const uint32_t k = pkeys[at], rel = prel[at];
        const int32_t sl = seller_slot(k, k != kEmpty32 ? s_sell[part_slot(k, log2nb, log2sell)] : 0u);
        if (sl >= 0) settle(k, rel, tp0 + i, sp_tbeg[i] + rel, atomicCAS(&s_own[sl], kEmpty32, sp_tbeg[i] + rel));
    }
    if (bad) atomicOr(err, bad);
}

// One flag byte per row -> the flag words and wave counts of scan.hpp's flag tiles (what the tile scan and the row emit read).
__global__ __launch_bounds__(kBlock) void q8_flag_pack_kernel(const uint8_t *__restrict__ flag_bytes, uint32_t *__restrict__ flag_words,
                                                              uint32_t *__restrict__ counts) {
    const uint32_t *b4 = reinterpret_cast<const uint32_t *>(flag_bytes + (size_t)blockIdx.x * kFlagTile + flag_rel0());
    uint32_t flags = 0;
#pragma unroll
    for (int it = 0; it < kFlagIters; ++it) {
        const uint32_t v = b4[it * 64];   // the lane's four rows of this 256-row group, a byte each (0 or 1)
        flags |= ((v & 1u) | ((v >> 7) & 2u) | ((v >> 14) & 4u) | ((v >> 21) & 8u)) << (it * 4);
    }
    store_flags_and_counts(flags, (int32_t)blockIdx.x, flag_words, counts);
}

// Range path: the persons arrive in any order, so "every flagged row is a DISTINCT (p_id, name)" is not given -- it holds when no
// two flagged persons of a window share an id, i.e. when the window's flagged ROWS are as many as the ids present in BOTH bitmaps
// (sellers S, persons P; both built with fire-and-forget ORs).  One workgroup per window counts popc(S & P) and compares; a window
// where they differ (duplicate ids -- equal or different names -- among the persons that sell) voids the call: the hash path decides.
__global__ __launch_bounds__(kBlock) void q8_unique_check_kernel(const WinBitmap *__restrict__ wins, const uint32_t *__restrict__ sellers,
                                                                 const uint32_t *__restrict__ persons, const int64_t *__restrict__ seg_out_off, uint32_t *err) {
    __shared__ uint64_t s_red[kWavesPerBlock];
    const WinBitmap wb = wins[blockIdx.x];
    const uint32_t n_words = (wb.n_bits + 31) >> 5;
    uint64_t n = 0;
    for (uint32_t i = threadIdx.x; i < n_words; i += kBlock) n += (uint64_t)__popc(sellers[wb.word_off + i] & persons[wb.word_off + i]);
    n = wave_sum_u64(n);
    if (lane_id() == 0) s_red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0 && s_red[0] + s_red[1] + s_red[2] + s_red[3] != (uint64_t)(seg_out_off[blockIdx.x + 1] - seg_out_off[blockIdx.x])) atomicOr(err, 1u);
}

// Dense-path layout decided on the device: window w gets a bitmap over [first p_id & ~31, last p_id] when it has at least as many
// bits as rows and at most 64 x rows + 4096 (the bound the host sized the arena for).  A window that does not qualify declines the
// whole call: every n_bits becomes 0 (no seller is recorded, no person flagged) and info[1] = 0 sends the host to the general path.
// First and last id: two loads per window instead of segment_stats_kernel's pass over the column:
// 0.033 ms per 2e7 persons); q8_persons_flag_kernel verifies that the ids are strictly increasing, which makes them minimum and maximum.
__global__ __launch_bounds__(kBlock) void q8_edge_layout_kernel(const int32_t *__restrict__ p_id, const int64_t *__restrict__ seg_off,
                                                                int32_t n_win, WinBitmap *__restrict__ wins, uint64_t *__restrict__ info) {
    __shared__ uint64_t s_wave[kWavesPerBlock];
    __shared__ uint64_t s_carry;
    int ok = 1;
    for (int32_t w = threadIdx.x; w < n_win; w += kBlock) {
        const int64_t lo = seg_off[2 * w], hi = seg_off[2 * w + 1];
        if (hi <= lo) continue;
        const int64_t base = (int64_t)p_id[lo] & ~int64_t(31), bits = (int64_t)p_id[hi - 1] - base + 1;
        if (bits < hi - lo || bits > 64 * (hi - lo) + 4096 || bits >= (int64_t(1) << 31)) ok = 0;
    }
    ok = __syncthreads_and(ok);
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    for (int32_t w0 = 0; w0 < n_win; w0 += kBlock) {
        const int32_t w = w0 + (int32_t)threadIdx.x;
        int64_t base = 0, bits = 0;
        if (ok && w < n_win && seg_off[2 * w + 1] > seg_off[2 * w]) {
            base = (int64_t)p_id[seg_off[2 * w]] & ~int64_t(31);
            bits = (int64_t)p_id[seg_off[2 * w + 1] - 1] - base + 1;
        }
        const uint64_t words = (uint64_t)((bits + 31) >> 5);
        const uint64_t incl = wave_incl_scan_u64(words);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint64_t off = s_carry + incl - words;
        for (int v = 0; v < wave; ++v) off += s_wave[v];
        if (w < n_win) wins[w] = WinBitmap{(int32_t)base, (uint32_t)bits, off};
        __syncthreads();
        if (threadIdx.x == kBlock - 1) s_carry = off + words;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        info[0] = s_carry;  // bitmap words in use
        info[1] = (uint64_t)ok;
    }
}

// bitmaps[0 .. info[0] + 4) = 0 (a bounded grid walks the words in use: a grid over the arena's bound is tens of thousands of
// workgroups that leave at once)
__global__ __launch_bounds__(kBlock) void q8_zero_bitmaps_kernel(uint32_t *__restrict__ bitmaps, const uint64_t *__restrict__ info) {
    const uint64_t n = info[0] + 4;
    for (uint64_t i = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * 4; i < n; i += (uint64_t)gridDim.x * kBlock * 4) {
        if (i + 4 <= n) *reinterpret_cast<uint4 *>(bitmaps + i) = make_uint4(0, 0, 0, 0);
        else
            for (uint64_t k = i; k < n; ++k) bitmaps[k] = 0;
    }
}

// ---- steady-state kernels of the gapless dense path (round 4) ------------------------------------------------------------------------
// persons: the bit test of q8_persons_flag_kernel with the layout derived in place, PLUS -- for the rows that join -- the bytes of their
// names: the tile's name offsets are read here (one 16-byte load per lane and iteration next to the p_id load: 4 B / row more of a
// pure stream) so that no separate length pass over the result rows is needed.  Per tile: counts[4] (rows per wave), bytes4[4]
// (name bytes per wave) and tile_tot {rows, bytes} for the emit pass's self-scan.
__global__ __launch_bounds__(kBlock) void q8_persons_flag_fast_kernel(const int32_t *__restrict__ p_id, const int32_t *__restrict__ name_off, int64_t n_rows,
                                                                      SegTiles st, const uint32_t *__restrict__ bitmaps, uint32_t *__restrict__ flag_words,
                                                                      uint32_t *__restrict__ counts, uint32_t *__restrict__ bytes4, uint2 *__restrict__ tile_tot,
                                                                      uint32_t *h_flags) {
    __shared__ uint32_t s_tot[2][kWavesPerBlock];
    const int32_t tile = (int32_t)blockIdx.x;
    const TileRange tr = locate_tile(st, tile, kFlagTile);
    const int32_t rel0 = flag_rel0();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    int32_t a[kFlagIters][4];
    load_flag_tile(p_id, n_rows, tr, a);
    const bool whole = tr.tile_begin >= 0 && tr.tile_begin + kFlagTile < n_rows;   // (block-uniform) every offset of the tile's rows + 1 exists
    int32_t off[kFlagIters][5], before[kFlagIters];
#pragma unroll
    for (int it = 0; it < kFlagIters; ++it) {
        const int64_t r0 = tr.tile_begin + rel0 + it * 256, chunk0 = r0 - lane * 4;
        const int64_t rb = chunk0 - 1;
        before[it] = p_id[rb < 0 ? 0 : (rb < n_rows ? rb : n_rows - 1)];
        if (whole) {
            const int4 o = *reinterpret_cast<const int4 *>(name_off + r0);   // (r0 is a multiple of 4; the host checked the column's alignment)
            off[it][0] = o.x; off[it][1] = o.y; off[it][2] = o.z; off[it][3] = o.w;
            const int32_t last = name_off[chunk0 + 256];
            const int32_t nxt = __shfl_down(off[it][0], 1, 64);
            off[it][4] = lane == 63 ? last : nxt;
        } else {
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int64_t r = r0 + j;
                off[it][j] = name_off[r < 0 ? 0 : (r > n_rows ? n_rows : r)];
            }
        }
    }
    // (the window's layout -- two dependent loads -- only after the tile's ids and offsets have been asked for)
    const GaplessWin g = gapless_window(p_id, st.seg_off, tr.seg, h_flags);
    const WinBitmap wb = g.wb;
    const int32_t rel_lo = (int32_t)(tr.lo - tr.tile_begin), rel_hi = (int32_t)(tr.hi - tr.tile_begin);
    const uint32_t *gbm = bitmaps + wb.word_off;
    uint32_t flags = 0, my_bytes = 0;
    bool bad = false;
#pragma unroll
    for (int it = 0; it < kFlagIters; ++it)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t rel = rel0 + it * 256 + j;
            const uint32_t idx = (uint32_t)a[it][j] - (uint32_t)wb.base;
            const bool row_in = rel >= rel_lo && rel < rel_hi;
            const bool in = row_in && idx < wb.n_bits;
            if (row_in && wb.n_bits) {   // strictly increasing, inside [first, last]: with "no gaps" the ids are exactly first .. last
                int32_t prev;
                if (j > 0) prev = a[it][j - 1];
                else {
                    prev = __shfl_up(a[it][3], 1, 64);
                    if (lane == 0) prev = before[it];
                }
                bad = bad || !(rel == rel_lo || a[it][j] > prev) || idx >= wb.n_bits;
            }
            const bool f = in & ((gbm[in ? idx >> 5 : 0u] >> (idx & 31)) & 1u);
            flags |= (f ? 1u : 0u) << (it * 4 + j);
            my_bytes += f ? (uint32_t)(off[it][j + 1] - off[it][j]) : 0u;
        }
    if (bad) __hip_atomic_store(h_flags, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    flag_words[(size_t)tile * kBlock + threadIdx.x] = flags;
    const uint32_t incl_r = wave_incl_scan_u32((uint32_t)__popc(flags)), incl_b = wave_incl_scan_u32(my_bytes);
    if (lane == 63) {
        counts[(size_t)tile * kWavesPerBlock + wave] = incl_r;
        bytes4[(size_t)tile * kWavesPerBlock + wave] = incl_b;
        s_tot[0][wave] = incl_r;
        s_tot[1][wave] = incl_b;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        tile_tot[tile] = make_uint2(s_tot[0][0] + s_tot[0][1] + s_tot[0][2] + s_tot[0][3], s_tot[1][0] + s_tot[1][1] + s_tot[1][2] + s_tot[1][3]);
}

// emit: EVERYTHING the query returns, in one pass over the person tiles -- person_row, p_id, name offsets and name bytes.  Every
// other person of a window sells (the join keeps half the rows), so the names are read the way they lie: a wave's 256 consecutive
// rows name one contiguous byte range (~3 KB), fetched with coalesced 16-byte loads into LDS; the names that join are packed in LDS
// and leave as 16-byte stores (the row-driven take read 32-byte sectors at random and needed a length pass, a scan and a row list
// first: 0.10 + 0.026 + 0.013 + 0.027 ms of q8's 0.30 ms at 1e9 events).  The workgroup finds its output position itself (sum of
// the lower tiles' totals), reports the windows' offsets and the totals straight into pinned host memory, and zeroes its rows'
// share of the seller bitmap for the next call (clean-up after use: no zeroing launch).
constexpr int kNameStage = 4096;   // bytes of names per 256 rows that fit the wave's LDS slots (16 B per row on average; beyond: the call is declined)
constexpr int kNameSlot = kNameStage + 48;   // (+ the in / out phase, and the dwords lds_copy_value reads past a value)
// One value from the staged source bytes to its place in the packed output, both in LDS, at any two byte alignments: the value's
// next 16 bytes come in as five ALIGNED dwords (an unaligned LDS read costs 6x) and are realigned in registers; they go out as the
// few bytes up to the destination's next dword boundary, whole aligned dwords, and the bytes behind the last whole dword -- ~10 LDS
// instructions for an 11-byte name where a byte-wise copy issued 18.
__device__ __forceinline__ void lds_copy_value(uint8_t *out_base, uint32_t dst, const uint32_t *src_words, uint32_t src, uint32_t len) {
    for (uint32_t done = 0; done < len; done += 16, src += 16, dst += 16) {
        const uint32_t n = min(16u, len - done), wi = src >> 2, sh = (src & 3) * 8;
        const uint32_t w0 = src_words[wi], w1 = src_words[wi + 1], w2 = src_words[wi + 2], w3 = src_words[wi + 3], w4 = src_words[wi + 4];
        uint32_t v[5] = {__funnelshift_r(w0, w1, sh), __funnelshift_r(w1, w2, sh), __funnelshift_r(w2, w3, sh), __funnelshift_r(w3, w4, sh), 0u};
        const uint32_t head = min(n, (4u - (dst & 3u)) & 3u);   // bytes up to the destination's dword boundary
        for (uint32_t c = 0; c < head; ++c) out_base[dst + c] = (uint8_t)(v[0] >> (8 * c));
        const uint32_t hs = head * 8, body = (n - head) >> 2;
        uint32_t *ow = reinterpret_cast<uint32_t *>(out_base + dst + head);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (k < body) ow[k] = __funnelshift_r(v[k], v[k + 1], hs);
        const uint32_t at = head + body * 4;   // bytes written so far; at most three more
        for (uint32_t c = at; c < n; ++c) out_base[dst + c] = (uint8_t)(v[c >> 2] >> (8 * (c & 3)));
    }
}
__global__ __launch_bounds__(kBlock) void q8_emit_fused_kernel(const int32_t *__restrict__ p_id, const int32_t *__restrict__ name_off,
                                                               const uint8_t *__restrict__ name, int64_t n_rows, SegTiles st,
                                                               const uint32_t *__restrict__ flag_words, const uint32_t *__restrict__ counts,
                                                               const uint32_t *__restrict__ bytes4, const uint2 *__restrict__ tile_tot, uint32_t *bitmaps,
                                                               int32_t *__restrict__ out_person_row, int32_t *__restrict__ out_p_id,
                                                               int32_t *__restrict__ out_off, uint8_t *__restrict__ out_bytes, uint64_t cap_rows,
                                                               uint64_t cap_bytes, int64_t *__restrict__ h_off, uint64_t *__restrict__ h_tot,
                                                               uint32_t *h_flags) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kWavesPerBlock][kNameSlot];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[kWavesPerBlock][kNameSlot];
    __shared__ uint16_t s_row[kWavesPerBlock][256], s_end[kWavesPerBlock][256], s_src[kWavesPerBlock][256];
    __shared__ uint64_t s_red[2 * kWavesPerBlock];
    const int32_t tile = (int32_t)blockIdx.x;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    // ---- where this tile's rows and bytes start: the lower tiles' totals, summed here (no scan launch)
    uint64_t sr = 0, sb = 0;
    for (int32_t t0 = (int32_t)threadIdx.x; t0 < tile; t0 += 4 * kBlock) {   // (four loads in flight per lane: the sum of 2442 tiles' totals was a chain of ten)
        uint2 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = t0 + k * kBlock < tile ? tile_tot[t0 + k * kBlock] : make_uint2(0, 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sr += v[k].x;
            sb += v[k].y;
        }
    }
    sr = wave_sum_u64(sr);
    sb = wave_sum_u64(sb);
    if (lane == 0) {
        s_red[wave] = sr;
        s_red[kWavesPerBlock + wave] = sb;
    }
    const TileRange tr = locate_tile(st, tile, kFlagTile);
    const GaplessWin g = gapless_window(p_id, st.seg_off, tr.seg, h_flags);
    __syncthreads();
    uint64_t base_rows = 0, base_bytes = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) {
        base_rows += s_red[w];
        base_bytes += s_red[kWavesPerBlock + w];
    }
    // ---- this tile's share of the bitmap goes back to zero (every tile of a window together covers the window's words)
    if (g.wb.n_bits) {
        const uint32_t idx_lo = (uint32_t)(g.first_id - g.wb.base) + (uint32_t)(tr.lo - g.lo), idx_hi = (uint32_t)(g.first_id - g.wb.base) + (uint32_t)(tr.hi - g.lo);
        uint32_t *gbm = bitmaps + g.wb.word_off;
        // (the window's first tile also clears the bits below the first id in the first word)
        const uint32_t w_lo = tr.lo == g.lo ? 0u : idx_lo >> 5;
        for (uint32_t wd = w_lo + threadIdx.x; wd <= ((idx_hi - 1) >> 5); wd += kBlock) gbm[wd] = 0;
    }
    const uint4 wc = *reinterpret_cast<const uint4 *>(counts + (size_t)tile * kWavesPerBlock);
    const uint4 wbv = *reinterpret_cast<const uint4 *>(bytes4 + (size_t)tile * kWavesPerBlock);
    const uint64_t tile_rows = (uint64_t)wc.x + wc.y + wc.z + wc.w, tile_bytes = (uint64_t)wbv.x + wbv.y + wbv.z + wbv.w;
    if (threadIdx.x == 0) {
        if (tile == st.tile_first[tr.seg]) h_off[tr.seg] = (int64_t)base_rows;
        if (tile == st.n_tiles - 1) {
            h_tot[0] = base_rows + tile_rows;
            h_tot[1] = base_bytes + tile_bytes;
        }
        if (tile == 0 && cap_rows) out_off[0] = 0;
    }
    if (base_rows + tile_rows > cap_rows || base_bytes + tile_bytes > cap_bytes) {   // (block-uniform) the hints were too small: the host redoes this pass
        if (threadIdx.x == 0) __hip_atomic_store(h_flags + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    if (tile_rows == 0) return;
    uint64_t cur_rows = base_rows + (wave > 0 ? wc.x : 0u) + (wave > 1 ? wc.y : 0u) + (wave > 2 ? wc.z : 0u);
    uint64_t cur_bytes = base_bytes + (wave > 0 ? wbv.x : 0u) + (wave > 1 ? wbv.y : 0u) + (wave > 2 ? wbv.z : 0u);
    const uint32_t flags = flag_words[(size_t)tile * kBlock + threadIdx.x];
    const int32_t rel0 = flag_rel0();
    const bool whole = tr.tile_begin >= 0 && tr.tile_begin + kFlagTile < n_rows;
    const uintptr_t name_addr = reinterpret_cast<uintptr_t>(name);
    uint8_t *in = s_in[wave], *outb = s_out[wave];
    uint16_t *lrow = s_row[wave], *lend = s_end[wave], *lsrc = s_src[wave];
    // the name offsets of all eight iterations are asked for up front: the iterations themselves then wait for one memory round trip
    // (their bytes), not for two in a row
    int4 o4[kFlagIters];
    int32_t olast[kFlagIters];
    if (whole) {
#pragma unroll
        for (int it = 0; it < kFlagIters; ++it) {
            const int64_t r0 = tr.tile_begin + rel0 + it * 256;
            o4[it] = *reinterpret_cast<const int4 *>(name_off + r0);
            olast[it] = name_off[r0 - lane * 4 + 256];
        }
    }
    // The bytes of iteration it + 1 are asked for (into registers) BEFORE iteration it is packed and written out: with four waves per
    // SIMD and every iteration a chain "names -> LDS -> pack -> store", a wave that waits for its names with nothing else in flight
    // left the memory system idle (0.19 ms for 0.55 GB; rocprofv3, round 4).
    constexpr int kStageLoads = (kNameStage + 16 + 1023) / 1024;   // 16-byte loads per lane that cover a full slot
    uint4 stg[kStageLoads];
    auto range_of = [&](int it, int32_t *b0, int32_t *b1) {   // (whole tiles) the byte range the wave's 256 rows of iteration `it` name
        *b0 = __builtin_amdgcn_readfirstlane(o4[it].x);
        *b1 = __builtin_amdgcn_readlane(olast[it], 63);
    };
    auto fetch = [&](int32_t b0, int32_t b1) {
        const uint32_t in_phase = (uint32_t)((name_addr + (uint32_t)b0) & 15), span = (uint32_t)(b1 - b0) + in_phase;
        // a 16-byte aligned chunk that holds at least one byte of the range never crosses a page: reading its tail is safe
        const uint4 *src = reinterpret_cast<const uint4 *>((name_addr + (uint32_t)b0) & ~uintptr_t(15));
#pragma unroll
        for (int k = 0; k < kStageLoads; ++k) {
            const uint32_t o = lane * 16 + k * 1024;
            stg[k] = (b1 > b0 && span <= (uint32_t)kNameStage + 16u && o < span) ? src[o >> 4] : make_uint4(0, 0, 0, 0);
        }
    };
    if (whole) {
        int32_t b0, b1;
        range_of(0, &b0, &b1);
        fetch(b0, b1);
    }
#pragma unroll
    for (int it = 0; it < kFlagIters; ++it) {
        const uint32_t f4 = (flags >> (it * 4)) & 15u;
        const int64_t r0 = tr.tile_begin + rel0 + it * 256;
        int32_t off[5];
        if (whole) {
            off[0] = o4[it].x; off[1] = o4[it].y; off[2] = o4[it].z; off[3] = o4[it].w;
            const int32_t nxt = __shfl_down(off[0], 1, 64);
            off[4] = lane == 63 ? olast[it] : nxt;
        } else {
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int64_t r = r0 + j;
                off[j] = name_off[r < 0 ? 0 : (r > n_rows ? n_rows : r)];
            }
        }
        const int32_t b0 = __builtin_amdgcn_readfirstlane(off[0]);
        const int32_t b1 = __builtin_amdgcn_readlane(off[4], 63);
        const uint32_t in_phase = (uint32_t)((name_addr + (uint32_t)b0) & 15);
        const uint32_t span = (uint32_t)(b1 - b0) + in_phase;
        const bool fits = b1 >= b0 && span <= (uint32_t)kNameStage + 16u;   // (wave-uniform)
        if (!whole && fits) fetch(b0, b1);   // (a ragged last tile: no pipelining)
        if (fits) {
#pragma unroll
            for (int k = 0; k < kStageLoads; ++k) {
                const uint32_t o = lane * 16 + k * 1024;
                if (b1 > b0 && o < span) *reinterpret_cast<uint4 *>(in + o) = stg[k];
            }
        }
        if (whole && it + 1 < kFlagIters) {   // the next iteration's names, on their way while this one is packed
            int32_t n0, n1;
            range_of(it + 1, &n0, &n1);
            fetch(n0, n1);
        }
        if (!__ballot(f4 != 0)) continue;   // (wave-uniform) none of these 256 persons sells
        if (!fits) {   // names too long for the slots: not this kernel's input
            if (lane == 0) __hip_atomic_store(h_flags, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            continue;
        }
        uint32_t len[4], mine_b = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            len[j] = (f4 >> j) & 1u ? (uint32_t)(off[j + 1] - off[j]) : 0u;
            mine_b += len[j];
        }
        const uint32_t mine_r = (uint32_t)__popc(f4);
        const uint32_t incl_b = wave_incl_scan_u32(mine_b), incl_r = wave_incl_scan_u32(mine_r);
        const uint32_t it_b = (uint32_t)__builtin_amdgcn_readlane((int)incl_b, 63), it_r = (uint32_t)__builtin_amdgcn_readlane((int)incl_r, 63);
        const uint32_t out_phase = (uint32_t)(cur_bytes & 15);
        __builtin_amdgcn_wave_barrier();   // the staged bytes are in place
        // the flagged rows line up in LDS lists (row, source position, end in the packed output) ...
        uint32_t pos = incl_b - mine_b, rk = incl_r - mine_r;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((f4 >> j) & 1u) {
                pos += len[j];
                lrow[rk] = (uint16_t)(rel0 + it * 256 + j);
                lsrc[rk] = (uint16_t)(in_phase + (uint32_t)(off[j] - b0));
                lend[rk] = (uint16_t)pos;
                ++rk;
            }
        __builtin_amdgcn_wave_barrier();
        // ... and are copied one value per lane, every lane busy (walking a lane's own four rows left half the lanes idle at every step)
        for (uint32_t i = lane; i < it_r; i += 64) {
            const uint32_t end_i = lend[i], start_i = i ? lend[i - 1] : 0u;
            lds_copy_value(outb, out_phase + start_i, reinterpret_cast<const uint32_t *>(in), lsrc[i], end_i - start_i);
        }
        __builtin_amdgcn_wave_barrier();
        // the packed names: LDS byte i is output byte (cur_bytes - out_phase) + i
        uint8_t *gout = out_bytes + (cur_bytes - out_phase);
        const uint32_t end = out_phase + it_b;
        for (uint32_t o = lane * 16; o < end; o += 64 * 16) {
            if (o >= out_phase && o + 16 <= end) {
                stream_store4(gout + o, *reinterpret_cast<const uint4 *>(outb + o));
            } else {   // the first / last chunk is shared with the neighbouring iteration, wave or tile: only this iteration's bytes
                for (uint32_t c = (o < out_phase ? out_phase : o); c < o + 16 && c < end; ++c) gout[c] = outb[c];
            }
        }
        for (uint32_t i = lane; i < it_r; i += 64) {
            const int64_t r = tr.tile_begin + lrow[i];
            stream_store(&out_person_row[cur_rows + i], (int32_t)r);
            stream_store(&out_p_id[cur_rows + i], g.first_id + (int32_t)(r - g.lo));   // no gaps: the id is arithmetic
            stream_store(&out_off[cur_rows + i + 1], (int32_t)(cur_bytes + lend[i]));   // (lend: the value's end inside this iteration's bytes)
        }
        __builtin_amdgcn_wave_barrier();   // the slots are rewritten by the next iteration
        cur_rows += it_r;
        cur_bytes += it_b;
    }
}

}  // namespace

extern "C" {

int flockgpu_q8_join(flockgpu_ctx *ctx, const flockgpu_person_cols *person, const flockgpu_windows *person_win,
                     const flockgpu_auction_cols *auction, const flockgpu_windows *auction_win, flockgpu_q8_result *out) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    if (!auction || !person || !out || auction->rows < 0 || person->rows < 0)
        return fail(ctx, FLOCKGPU_ERR_INVALID, "q8: null argument");
    FG_TRY(check_windows(ctx, auction_win, auction->rows, "q8.auction"));
    FG_TRY(check_windows(ctx, person_win, person->rows, "q8.person"));
    if (auction_win->n_windows != person_win->n_windows)
        return fail(ctx, FLOCKGPU_ERR_INVALID, "q8: auction and person schedules differ in window count");
    if (auction->rows >= (int64_t(1) << 31) || person->rows >= (int64_t(1) << 31) - 1)
        return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "q8: relations are limited to 2^31 rows per call");
    if (auction->rows > 0 && !auction->seller) return fail(ctx, FLOCKGPU_ERR_INVALID, "q8: null seller column");
    if (person->rows > 0 && (!person->p_id || !person->name.offsets || !person->name.data))
        return fail(ctx, FLOCKGPU_ERR_INVALID, "q8: null person column");
    if ((reinterpret_cast<uintptr_t>(auction->seller) & 15) || (reinterpret_cast<uintptr_t>(person->p_id) & 15))
        return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "q8: seller and p_id columns must be 16-byte aligned");
    FG_HIP(ctx, hipSetDevice(ctx->device));
    const int n_win = auction_win->n_windows;

    std::vector<int64_t> ab(n_win), ae(n_win), pb(n_win), pe(n_win);
    int64_t max_p = 0, max_a = 0, out_cap = 16;
    for (int w = 0; w < n_win; ++w) {
        ab[w] = auction_win->pane_row_offsets[auction_win->win_pane_lo[w]];
        ae[w] = auction_win->pane_row_offsets[auction_win->win_pane_hi[w]];
        pb[w] = person_win->pane_row_offsets[person_win->win_pane_lo[w]];
        pe[w] = person_win->pane_row_offsets[person_win->win_pane_hi[w]];
        max_p = std::max(max_p, pe[w] - pb[w]);
        max_a = std::max(max_a, ae[w] - ab[w]);
        out_cap += pe[w] - pb[w];
    }
    SegTiles st_a, st_p;
    FG_TRY(build_seg_tiles(ctx, "q8.auction", ab.data(), ae.data(), n_win, kFlagTile, &st_a));
    FG_TRY(build_seg_tiles(ctx, "q8.person", pb.data(), pe.data(), n_win, kFlagTile, &st_p));

    // per-window key statistics of the persons: {min, max, sorted} x n_win (exact, on the device)
    int32_t *d_stats = nullptr, *h_stats = nullptr;
    FG_TRY(arena_get_t(ctx, "q8.stats", (size_t)3 * std::max(n_win, 1), &d_stats));
    FG_TRY(pinned_get_t(ctx, "q8.stats", (size_t)3 * std::max(n_win, 1), &h_stats));
    uint32_t *flag_words = nullptr, *counts = nullptr;
    uint64_t *tile_base = nullptr;
    FG_TRY(arena_get_t(ctx, "q8.flag_words", (size_t)st_p.n_tiles * kBlock, &flag_words));
    FG_TRY(arena_get_t(ctx, "q8.counts", (size_t)st_p.n_tiles * kWavesPerBlock + 4, &counts));
    FG_TRY(arena_get_t(ctx, "q8.tile_base", (size_t)st_p.n_tiles + 1, &tile_base));
    int64_t *d_off = nullptr, *h_off = nullptr;
    FG_TRY(arena_get_t(ctx, "q8.seg_out_off", (size_t)n_win + 1, &d_off));
    FG_TRY(pinned_get_t(ctx, "q8.seg_out_off", (size_t)n_win + 2, &h_off));
    int32_t *o_pr = nullptr;
    FG_TRY(arena_get_t(ctx, "q8.out_person_row", (size_t)out_cap, &o_pr));  // at most every person of every window
    std::vector<int64_t> &offs = ctx->host_i64["q8.win_out_offsets"];
    Utf8Gather g_name;
    int64_t n_out = 0;

    // As in q3: the dense path is speculated -- a device pass lays the bitmaps out, everything up to the name lengths is
    // queued behind it, and the verdict, the row counts and the byte total reach the host in ONE synchronisation
    // (four before).  After a call that did not qualify the statistics are read first.
    // regime of the ctx's last call: 1 = dense, ordered ids (speculated: where a ctx starts); 2 = dense RANGE, ids in any order (exact
    // statistics first); 0 = hash tables
    std::vector<int64_t> &regime = ctx->host_i64["q8.dense_regime"];
    if (regime.empty()) regime.push_back(1);
    // exact statistics of the persons' ids, one more wait: every window strictly increasing over an affordable range -> 1; an affordable
    // range in any order -> 2 (bitmaps over [min, max] need no order: interleaved generators, Kafka partitions, a shuffled replay --
    // ids that are dense but not time-ordered); else 0
    auto look = [&](int *mode_out) -> int {
        FG_TRY(segment_key_stats(ctx, person->p_id, person->rows, st_p, d_stats, d_stats + n_win, d_stats + 2 * n_win));
        FG_HIP(ctx, hipMemcpyAsync(h_stats, d_stats, sizeof(int32_t) * 3 * n_win, hipMemcpyDeviceToHost, ctx->stream));
        FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        bool ordered = true, affordable = true;
        for (int w = 0; w < n_win; ++w) {
            if (pe[w] == pb[w]) continue;
            const int64_t base = (int64_t)h_stats[w] & ~int64_t(31), bits = (int64_t)h_stats[n_win + w] - base + 1;
            ordered = ordered && h_stats[2 * n_win + w];
            affordable = affordable && bits <= 64 * (pe[w] - pb[w]) + 4096 && bits < (int64_t(1) << 31);
        }
        *mode_out = affordable ? (ordered ? 1 : 2) : 0;
        return FLOCKGPU_OK;
    };
    int mode = n_win > 0 ? (int)regime[0] : 0;
    if (n_win > 0 && mode != 1) FG_TRY(look(&mode));   // the previous call did not qualify for the speculated path: look before building
    bool try_dense = mode == 1;
    // ---- the steady-state sequence of the gapless dense path: sellers (layout inline) -> persons (+ name lengths) -> emit (rows, ids,
    // name offsets AND bytes; self-scan; zeroes the bitmap behind itself): THREE launches and ONE synchronisation, nothing else on the
    // stream -- no memset / copy nodes (flags, window offsets and totals land in one pinned block), no scan launches, no separate Utf8
    // length / take passes, no id gather.  Taken once a call of this ctx has gone through the general sequence below (which leaves the
    // output-size estimates); anything unusual -- ids with gaps or out of order, long names, estimates too small beyond one retry --
    // falls through to it again.
    std::vector<int64_t> &fast = ctx->host_i64["q8.fast_hint"];   // {row capacity, byte capacity, valid, calls to skip after a decline, bitmap words known zero}
    if (fast.size() != 5) fast.assign(5, 0);
    if (fast[3] > 0) --fast[3];
    const bool fast_ok = try_dense && regime[0] == 1 && fast[2] && fast[3] == 0 && st_a.n_tiles > 0 && st_p.n_tiles > 0 && st_p.n_tiles <= kSelfScanMaxTiles &&
                         (reinterpret_cast<uintptr_t>(person->name.offsets) & 15) == 0;
    if (fast_ok) {
        const size_t words = (size_t)(person->rows >> 5) + (size_t)2 * n_win + 8;
        uint32_t *bits = nullptr, *bytes4 = nullptr;
        uint2 *tile_tot = nullptr;
        uint64_t *h_blk = nullptr;
        const void *bits_before = ctx->arena["q8.fast_bits"].ptr;
        FG_TRY(arena_get_t(ctx, "q8.fast_bits", words, &bits));
        if (bits != bits_before || fast[4] < (int64_t)words) {   // a new (or grown) arena, or a call that may have left bits behind
            FG_HIP(ctx, hipMemsetAsync(bits, 0, sizeof(uint32_t) * words, ctx->stream));
        }
        fast[4] = 0;   // (set again when this call's emit pass has cleaned up behind itself)
        FG_TRY(arena_get_t(ctx, "q8.bytes4", (size_t)st_p.n_tiles * kWavesPerBlock + 4, &bytes4));
        FG_TRY(arena_get_t(ctx, "q8.tile_tot", (size_t)st_p.n_tiles + 1, &tile_tot));
        FG_TRY(pinned_get_t(ctx, "q8.fast", (size_t)n_win + 8, &h_blk));   // [0]: two flag words, [1] rows, [2] bytes, [4 ..] window offsets
        uint32_t *h_flags = reinterpret_cast<uint32_t *>(h_blk);
        int64_t *h_woff = reinterpret_cast<int64_t *>(h_blk + 4);
        h_blk[0] = h_blk[1] = h_blk[2] = 0;   // (the previous call's values were read under its synchronisation)
        {
            LaunchScope ls(ctx, "q8_sellers_bitmap_kernel");
            hipLaunchKernelGGL(q8_sellers_bitmap_inline_kernel, dim3((unsigned)st_a.n_tiles), dim3(kBlock), 0, ctx->stream, auction->seller, auction->rows, st_a,
                               person->p_id, st_p.seg_off, bits, h_flags);
        }
        FG_TRY(check_launch(ctx, "q8_sellers_bitmap_inline_kernel"));
        {
            LaunchScope ls(ctx, "q8_persons_flag_kernel");
            hipLaunchKernelGGL(q8_persons_flag_fast_kernel, dim3((unsigned)st_p.n_tiles), dim3(kBlock), 0, ctx->stream, person->p_id, person->name.offsets,
                               person->rows, st_p, bits, flag_words, counts, bytes4, tile_tot, h_flags);
        }
        FG_TRY(check_launch(ctx, "q8_persons_flag_fast_kernel"));
        int64_t cap_rows = std::min<int64_t>(out_cap - 16, std::max<int64_t>(fast[0], 1)), cap_bytes = std::max<int64_t>(fast[1], 16);
        bool done = false;
        for (int attempt = 0; attempt < 2 && !done; ++attempt) {
            int32_t *o_pid = nullptr, *o_off = nullptr;
            uint8_t *o_bytes = nullptr;
            FG_TRY(arena_get_t(ctx, "q8.out_p_id", (size_t)cap_rows + 1, &o_pid));
            FG_TRY(arena_get_t(ctx, "q8.fast_name_off", (size_t)cap_rows + 2, &o_off));
            FG_TRY(arena_get_t(ctx, "q8.fast_name_bytes", (size_t)cap_bytes + 32, &o_bytes));
            h_flags[1] = 0;
            {
                LaunchScope ls(ctx, "q8_emit_fused_kernel");
                hipLaunchKernelGGL(q8_emit_fused_kernel, dim3((unsigned)st_p.n_tiles), dim3(kBlock), 0, ctx->stream, person->p_id, person->name.offsets,
                                   person->name.data, person->rows, st_p, flag_words, counts, bytes4, tile_tot, bits, o_pr, o_pid, o_off, o_bytes,
                                   (uint64_t)cap_rows, (uint64_t)cap_bytes, h_woff, h_blk + 1, h_flags);
            }
            FG_TRY(check_launch(ctx, "q8_emit_fused_kernel"));
            FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (h_flags[0]) break;   // not this kernel's input: the general sequence decides
            fast[4] = (int64_t)words;   // every tile's emit workgroup zeroed its share before anything else
            if (h_flags[1]) {   // more rows / bytes than the estimates: the exact totals are known now, once more
                cap_rows = (int64_t)h_blk[1] + 16;
                cap_bytes = (int64_t)h_blk[2] + 16;
                continue;
            }
            n_out = (int64_t)h_blk[1];
            offs.assign((size_t)n_win + 1, 0);
            offs[(size_t)n_win] = n_out;
            for (int w = n_win - 1; w >= 0; --w) offs[(size_t)w] = pe[w] > pb[w] ? h_woff[w] : offs[(size_t)w + 1];
            fast[0] = n_out + n_out / 8 + 4096;
            fast[1] = (int64_t)h_blk[2] + (int64_t)h_blk[2] / 8 + 65536;
            out->p_id = o_pid;
            out->name = flockgpu_utf8{o_off, o_bytes};
            out->name_bytes = (int64_t)h_blk[2];
            out->person_row = o_pr;
            out->win_out_offsets = offs.data();
            out->rows = n_out;
            done = true;
        }
        if (done) return FLOCKGPU_OK;
        fast[2] = 0;
        fast[3] = 16;   // a declined call costs three launches and a wait for nothing: not again right away
    }
    if (try_dense) {
        const size_t bound_words = (size_t)2 * (size_t)person->rows + (size_t)130 * n_win + 8;
        WinBitmap *d_wins = nullptr;
        uint32_t *bitmaps = nullptr;
        uint64_t *d_info = nullptr, *h_info = nullptr;
        FG_TRY(arena_get_t(ctx, "q8.wins", (size_t)n_win, &d_wins));
        FG_TRY(arena_get_t(ctx, "q8.bitmaps", bound_words, &bitmaps));
        FG_TRY(arena_get_t(ctx, "q8.layout_info", 2, &d_info));
        FG_TRY(pinned_get_t(ctx, "q8.layout_info", 2, &h_info));
        uint32_t *d_verr = nullptr, *h_verr = nullptr;
        FG_TRY(arena_get_t(ctx, "q8.order_err", 4, &d_verr));
        FG_TRY(pinned_get_t(ctx, "q8.order_err", 4, &h_verr));
        FG_HIP(ctx, hipMemsetAsync(d_verr, 0, sizeof(uint32_t), ctx->stream));
        hipLaunchKernelGGL(q8_edge_layout_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, person->p_id, st_p.seg_off, n_win, d_wins, d_info);
        FG_TRY(check_launch(ctx, "q8_edge_layout_kernel"));
        hipLaunchKernelGGL(q8_zero_bitmaps_kernel, dim3((unsigned)std::min<int64_t>(div_up((int64_t)bound_words, kBlock * 4), 4096)), dim3(kBlock), 0,
                           ctx->stream, bitmaps, d_info);
        FG_TRY(check_launch(ctx, "q8_zero_bitmaps_kernel"));
        if (st_a.n_tiles > 0) {
            LaunchScope ls(ctx, "q8_sellers_bitmap_kernel");
            hipLaunchKernelGGL(q8_sellers_bitmap_kernel, dim3((unsigned)st_a.n_tiles), dim3(kBlock), 0, ctx->stream,
                               auction->seller, auction->rows, st_a, d_wins, bitmaps);
        }
        FG_TRY(check_launch(ctx, "q8_sellers_bitmap_kernel"));
        if (st_p.n_tiles > 0) {
            LaunchScope ls(ctx, "q8_persons_flag_kernel");
            const unsigned grid = (unsigned)std::min<int64_t>(st_p.n_tiles, (int64_t)ctx->num_cus * kStreamBlocksPerCu);
            hipLaunchKernelGGL(q8_persons_flag_kernel<true>, dim3(grid), dim3(kBlock), 0, ctx->stream, person->p_id, person->rows,
                               st_p, d_wins, bitmaps, flag_words, counts, d_verr);
        }
        FG_TRY(check_launch(ctx, "q8_persons_flag_kernel"));
        FG_TRY(launch_tile_scan(ctx, counts, st_p.n_tiles, tile_base, st_p.tile_first, st_p.n_seg, d_off));
        FG_TRY(emit_flagged_rows(ctx, st_p, flag_words, counts, tile_base, o_pr));
        // (the take of the names is laid out for the previous call's row count + 1/8, not for "every person": q3.hip does the same)
        std::vector<int64_t> &rows_hint = ctx->host_i64["q8.rows_hint"];
        if (rows_hint.empty()) rows_hint.push_back(0);
        const int64_t take_rows = rows_hint[0] > 0 ? std::min<int64_t>(out_cap - 16, rows_hint[0]) : out_cap - 16;
        FG_TRY(gather_utf8_begin(ctx, "q8.out_name", person->name, o_pr, take_rows, &g_name, tile_base + st_p.n_tiles));
        FG_HIP(ctx, hipMemcpyAsync(h_off, d_off, sizeof(int64_t) * ((size_t)n_win + 1), hipMemcpyDeviceToHost, ctx->stream));
        FG_HIP(ctx, hipMemcpyAsync(h_info, d_info, sizeof(uint64_t) * 2, hipMemcpyDeviceToHost, ctx->stream));
        FG_HIP(ctx, hipMemcpyAsync(h_verr, d_verr, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (*h_verr) h_info[1] = 0;   // some window's ids are not strictly increasing: the bitmaps' bounds and the DISTINCT shortcut are void
        if (h_info[1]) {
            offs.assign(h_off, h_off + n_win + 1);
            n_out = offs[n_win];
            if (n_out > take_rows) {   // more rows than the take was laid out for: once more, exactly
                FG_TRY(gather_utf8_begin(ctx, "q8.out_name", person->name, o_pr, n_out, &g_name, nullptr));
                FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
            }
            gather_utf8_narrow(&g_name, n_out);
            rows_hint[0] = n_out + n_out / 8 + 4096;
        } else {
            try_dense = false;
        }
    }
    if (!try_dense && mode == 1) FG_TRY(look(&mode));   // the speculation was declined: the statistics say what the ids are like
    if (!try_dense && mode == 1) mode = 0;               // (ordered and affordable by the statistics, yet declined: not an input for the bitmaps)
    if (mode == 2) {
        // ---- the RANGE path: bitmaps over every window's exact [min, max], persons in any order.  Sellers S and persons P are both
        // built with the LDS-staged fire-and-forget ORs of the dense path; a person is flagged when its id is in S; the flagged rows are
        // DISTINCT when rows = popc(S & P) per window (q8_unique_check_kernel) -- duplicates among the persons that sell send the call
        // to the hash tables.  No hashing, no compare-and-swap: the persons shuffled inside every window ran 2.0 ms per 1e9 events
        // through the hash path (the seller set alone 0.64 ms: 6.6e6 returning CAS on a 240 MB set, 4.7 % of the HBM rate).
        std::vector<WinBitmap> h_wins((size_t)n_win);
        uint64_t words = 0;
        for (int w = 0; w < n_win; ++w) {
            if (pe[w] == pb[w]) {
                h_wins[(size_t)w] = WinBitmap{0, 0u, words};
                continue;
            }
            const int32_t base = h_stats[w] & ~31;
            const uint32_t bits = (uint32_t)((int64_t)h_stats[n_win + w] - base + 1);
            h_wins[(size_t)w] = WinBitmap{base, bits, words};
            words += (bits + 31) >> 5;
        }
        WinBitmap *d_wins = nullptr, *p_wins = nullptr;
        uint32_t *sellers = nullptr, *present = nullptr, *d_err = nullptr, *h_err = nullptr;
        FG_TRY(arena_get_t(ctx, "q8.wins", (size_t)n_win, &d_wins));
        FG_TRY(pinned_get_t(ctx, "q8.wins", (size_t)n_win, &p_wins));
        FG_TRY(arena_get_t(ctx, "q8.bitmaps", (size_t)words + 8, &sellers));
        FG_TRY(arena_get_t(ctx, "q8.person_bits", (size_t)words + 8, &present));
        FG_TRY(arena_get_t(ctx, "q8.order_err", 4, &d_err));
        FG_TRY(pinned_get_t(ctx, "q8.order_err", 4, &h_err));
        std::copy(h_wins.begin(), h_wins.end(), p_wins);   // (the staging was last read under the statistics' synchronisation)
        FG_HIP(ctx, hipMemcpyAsync(d_wins, p_wins, sizeof(WinBitmap) * (size_t)n_win, hipMemcpyHostToDevice, ctx->stream));
        FG_HIP(ctx, hipMemsetAsync(sellers, 0, sizeof(uint32_t) * ((size_t)words + 4), ctx->stream));
        FG_HIP(ctx, hipMemsetAsync(present, 0, sizeof(uint32_t) * ((size_t)words + 4), ctx->stream));
        FG_HIP(ctx, hipMemsetAsync(d_err, 0, sizeof(uint32_t), ctx->stream));
        if (st_a.n_tiles > 0) {
            LaunchScope ls(ctx, "q8_sellers_bitmap_kernel");
            hipLaunchKernelGGL(q8_key_bitmap_wide_kernel, dim3((unsigned)div_up(st_a.n_tiles, kWideTiles)), dim3(kBlock), 0, ctx->stream, auction->seller, auction->rows, st_a, d_wins,
                               sellers);
        }
        FG_TRY(check_launch(ctx, "q8_sellers_bitmap_kernel"));
        if (st_p.n_tiles > 0) {
            {
                LaunchScope ls(ctx, "q8_person_bitmap_wide_kernel");
                hipLaunchKernelGGL(q8_person_bitmap_wide_kernel, dim3((unsigned)div_up(st_p.n_tiles, kWideTiles)), dim3(kBlock), 0, ctx->stream, person->p_id, person->rows, st_p,
                                   d_wins, present);
            }
            FG_TRY(check_launch(ctx, "q8_person_bitmap_wide_kernel"));
            LaunchScope ls(ctx, "q8_persons_flag_kernel");
            const unsigned grid = (unsigned)std::min<int64_t>(st_p.n_tiles, (int64_t)ctx->num_cus * kStreamBlocksPerCu);
            hipLaunchKernelGGL(q8_persons_flag_kernel<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, person->p_id, person->rows, st_p, d_wins, sellers, flag_words,
                               counts, d_err);
        }
        FG_TRY(check_launch(ctx, "q8_persons_flag_kernel"));
        FG_TRY(launch_tile_scan(ctx, counts, st_p.n_tiles, tile_base, st_p.tile_first, st_p.n_seg, d_off));
        hipLaunchKernelGGL(q8_unique_check_kernel, dim3((unsigned)n_win), dim3(kBlock), 0, ctx->stream, d_wins, sellers, present, d_off, d_err);
        FG_TRY(check_launch(ctx, "q8_unique_check_kernel"));
        FG_TRY(emit_flagged_rows(ctx, st_p, flag_words, counts, tile_base, o_pr));
        std::vector<int64_t> &rows_hint = ctx->host_i64["q8.rows_hint"];
        if (rows_hint.empty()) rows_hint.push_back(0);
        const int64_t take_rows = rows_hint[0] > 0 ? std::min<int64_t>(out_cap - 16, rows_hint[0]) : out_cap - 16;
        FG_TRY(gather_utf8_begin(ctx, "q8.out_name", person->name, o_pr, take_rows, &g_name, tile_base + st_p.n_tiles));
        FG_HIP(ctx, hipMemcpyAsync(h_off, d_off, sizeof(int64_t) * ((size_t)n_win + 1), hipMemcpyDeviceToHost, ctx->stream));
        FG_HIP(ctx, hipMemcpyAsync(h_err, d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (*h_err) {
            mode = 0;   // duplicate ids among the persons that sell: DISTINCT (p_id, name) needs the names compared
        } else {
            offs.assign(h_off, h_off + n_win + 1);
            n_out = offs[n_win];
            if (n_out > take_rows) {
                FG_TRY(gather_utf8_begin(ctx, "q8.out_name", person->name, o_pr, n_out, &g_name, nullptr));
                FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
            }
            gather_utf8_narrow(&g_name, n_out);
            rows_hint[0] = n_out + n_out / 8 + 4096;
        }
    }
    bool parted = false;
    if (mode == 0 && st_a.n_tiles > 0 && st_p.n_tiles > 0) {
        // ---- the hash path with both relations grouped by (window, hash bucket): every table in LDS (kernels above).  The bucket count
        // is sized for the LARGEST window's averages; a bucket that overflows its LDS tables voids the attempt (the global tables
        // below decide) and keeps this ctx off the partitioned path for a while.
        std::vector<int64_t> &skip = ctx->host_i64["q8.part_skip"];
        if (skip.empty()) skip.push_back(0);
        int log2nb = 0;
        while (log2nb < kPartMaxLog2 && ((max_p >> log2nb) > kPartPersonsPerBucket || (max_a >> log2nb) > kPartAuctionsPerBucket)) ++log2nb;
        const bool fits = (max_p >> log2nb) <= kPartPersonsPerBucket && (max_a >> log2nb) <= kPartAuctionsPerBucket &&
                          ((int64_t)n_win << log2nb) < (int64_t(1) << 30) && div_up(max_p, (int64_t)kFlagTile) + 1 <= kJoinChunk;
        // {a call of this ctx needed the large seller sets, calls since}: one workgroup per CU instead of three, so the small sets are
        // tried again now and then (a miss costs one more launch of the join)
        std::vector<int64_t> &large = ctx->host_i64["q8.part_large_set"];
        if (large.size() != 2) large.assign(2, 0);
        if (large[0] && ++large[1] >= 64) large[0] = large[1] = 0;
        if (skip[0] > 0) {
            --skip[0];
        } else if (fits) {
            const int nb = 1 << log2nb;
            uint32_t *skeys = nullptr, *pkeys = nullptr, *d_err = nullptr;
            uint16_t *soff = nullptr, *poff = nullptr, *prel = nullptr;
            uint8_t *flag_bytes = nullptr;
            FG_TRY(arena_get_t(ctx, "q8.part_skeys", (size_t)st_a.n_tiles * kFlagTile, &skeys));
            FG_TRY(arena_get_t(ctx, "q8.part_soff", (size_t)st_a.n_tiles * (size_t)(nb + 1) + 8, &soff));
            FG_TRY(arena_get_t(ctx, "q8.part_pkeys", (size_t)st_p.n_tiles * kFlagTile, &pkeys));
            FG_TRY(arena_get_t(ctx, "q8.part_prel", (size_t)st_p.n_tiles * kFlagTile, &prel));
            FG_TRY(arena_get_t(ctx, "q8.part_poff", (size_t)st_p.n_tiles * (size_t)(nb + 1) + 8, &poff));
            FG_TRY(arena_get_t(ctx, "q8.part_flag_bytes", (size_t)st_p.n_tiles * kFlagTile, &flag_bytes));
            FG_TRY(arena_get_t(ctx, "q8.err", 4, &d_err));
            FG_HIP(ctx, hipMemsetAsync(d_err, 0, sizeof(uint32_t), ctx->stream));
            {
                LaunchScope ls(ctx, "q8_sellers_part_kernel");
                hipLaunchKernelGGL(q8_sellers_part_kernel, dim3((unsigned)st_a.n_tiles), dim3(kBlock), 0, ctx->stream, auction->seller, auction->rows, st_a,
                                   log2nb, skeys, soff);
            }
            FG_TRY(check_launch(ctx, "q8_sellers_part_kernel"));
            {
                LaunchScope ls(ctx, "q8_persons_part_kernel");
                hipLaunchKernelGGL(q8_persons_part_kernel, dim3((unsigned)st_p.n_tiles), dim3(kBlock), 0, ctx->stream, person->p_id, person->rows, st_p, log2nb,
                                   pkeys, prel, poff, flag_bytes);
            }
            FG_TRY(check_launch(ctx, "q8_persons_part_kernel"));
            std::vector<int64_t> &rows_hint = ctx->host_i64["q8.rows_hint"];
            if (rows_hint.empty()) rows_hint.push_back(0);
            const int64_t take_rows = rows_hint[0] > 0 ? std::min<int64_t>(out_cap - 16, rows_hint[0]) : out_cap - 16;
            uint32_t perr = 0;
            for (int attempt = 0; attempt < 2; ++attempt) {
                const int log2sell = large[0] ? kJoinSellLog2Large : kJoinSellLog2;
                const size_t lds_bytes = sizeof(uint32_t) * ((size_t(2) << log2sell) + 4);
                if (large[0])
                    FG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&q8_bucket_join_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                    (int)lds_bytes));
                {
                    LaunchScope ls(ctx, "q8_bucket_join_kernel");
                    hipLaunchKernelGGL(q8_bucket_join_kernel, dim3((unsigned)((int64_t)n_win << log2nb)), dim3(kJoinBlock), lds_bytes, ctx->stream, person->p_id, person->name.offsets, person->name.data, st_a, st_p, log2nb, skeys, soff, pkeys, prel,
                                       poff, flag_bytes, log2sell, d_err);
                }
                FG_TRY(check_launch(ctx, "q8_bucket_join_kernel"));
                hipLaunchKernelGGL(q8_flag_pack_kernel, dim3((unsigned)st_p.n_tiles), dim3(kBlock), 0, ctx->stream, flag_bytes, flag_words, counts);
                FG_TRY(check_launch(ctx, "q8_flag_pack_kernel"));
                FG_TRY(launch_tile_scan(ctx, counts, st_p.n_tiles, tile_base, st_p.tile_first, st_p.n_seg, d_off));
                FG_TRY(emit_flagged_rows(ctx, st_p, flag_words, counts, tile_base, o_pr));
                FG_TRY(gather_utf8_begin(ctx, "q8.out_name", person->name, o_pr, take_rows, &g_name, tile_base + st_p.n_tiles));
                FG_HIP(ctx, hipMemcpyAsync(h_off, d_off, sizeof(int64_t) * ((size_t)n_win + 1), hipMemcpyDeviceToHost, ctx->stream));
                FG_HIP(ctx, hipMemcpyAsync(h_off + n_win + 1, d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
                FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
                perr = *reinterpret_cast<uint32_t *>(h_off + n_win + 1);
                if (perr != kPartErrSellers || large[0]) break;
                // only seller sets overflowed, and only the small ones were tried: the grouped lists stand, the join alone runs again
                large[0] = 1;
                large[1] = 0;
                FG_HIP(ctx, hipMemsetAsync(d_err, 0, sizeof(uint32_t), ctx->stream));
                FG_HIP(ctx, hipMemsetAsync(flag_bytes, 0, (size_t)st_p.n_tiles * kFlagTile, ctx->stream));
            }
            if (perr) {
                skip[0] = 16;
            } else {
                offs.assign(h_off, h_off + n_win + 1);
                n_out = offs[n_win];
                if (n_out > take_rows) {
                    FG_TRY(gather_utf8_begin(ctx, "q8.out_name", person->name, o_pr, n_out, &g_name, nullptr));
                    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
                }
                gather_utf8_narrow(&g_name, n_out);
                rows_hint[0] = n_out + n_out / 8 + 4096;
                parted = true;
            }
        }
    }
    if (mode == 0 && !parted) {
        const uint64_t pcap64 = std::max<uint64_t>(64, (uint64_t)max_p * 3 / 2 + 8);
        if (pcap64 >= (uint64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "q8: window too large");
        const uint32_t pcap = (uint32_t)pcap64;
        uint32_t *ptabs = nullptr, *d_err = nullptr;
        FG_TRY(arena_get_t(ctx, "q8.person_tables", (size_t)pcap * std::max(n_win, 1), &ptabs));
        FG_TRY(arena_get_t(ctx, "q8.err", 4, &d_err));
        // the seller sets are sized from the distinct-seller density seen last time; a full set redoes the batch
        uint64_t scap64 = std::max<uint64_t>(64, (uint64_t)((double)max_a / std::max(1.0, ctx->q8_rows_per_seller) * 2.0) + 64);
        for (int attempt = 0;; ++attempt) {
            if (attempt > 6 || scap64 >= (uint64_t(1) << 31))
                return fail(ctx, FLOCKGPU_ERR_CAPACITY, "q8: seller set capacity %llu still overflows", (unsigned long long)scap64);
            const uint32_t scap = (uint32_t)scap64;
            uint64_t *sets = nullptr;
            FG_TRY(arena_get_t(ctx, "q8.seller_sets", (size_t)scap * std::max(n_win, 1), &sets));
            FG_HIP(ctx, hipMemsetAsync(sets, 0xFF, sizeof(uint64_t) * (size_t)scap * n_win, ctx->stream));
            FG_HIP(ctx, hipMemsetAsync(ptabs, 0xFF, sizeof(uint32_t) * (size_t)pcap * n_win, ctx->stream));
            FG_HIP(ctx, hipMemsetAsync(d_err, 0, sizeof(uint32_t), ctx->stream));
            if (st_a.n_tiles > 0) {
                LaunchScope ls(ctx, "q8_sellers_set_kernel");
                hipLaunchKernelGGL(q8_sellers_set_kernel, dim3((unsigned)st_a.n_tiles), dim3(kBlock), 0, ctx->stream,
                                   auction->seller, auction->rows, st_a, sets, scap, d_err);
            }
            FG_TRY(check_launch(ctx, "q8_sellers_set_kernel"));
            if (st_p.n_tiles > 0) {
                LaunchScope ls(ctx, "q8_persons_general_kernel");
                hipLaunchKernelGGL(q8_persons_general_kernel, dim3((unsigned)st_p.n_tiles), dim3(kBlock), 0, ctx->stream,
                                   person->p_id, person->rows, person->name.offsets, person->name.data, st_p, ptabs, pcap, sets, scap,
                                   flag_words, counts, d_err);
            }
            FG_TRY(check_launch(ctx, "q8_persons_general_kernel"));
            FG_HIP(ctx, hipMemcpyAsync(h_off + n_win + 1, d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (*reinterpret_cast<uint32_t *>(h_off + n_win + 1)) {
                scap64 *= 4;
                continue;
            }
            if (attempt > 0) ctx->q8_rows_per_seller = std::max(1.0, (double)max_a * 2.0 / (double)scap64);
            break;
        }
        FG_TRY(launch_tile_scan(ctx, counts, st_p.n_tiles, tile_base, st_p.tile_first, st_p.n_seg, d_off));
        FG_TRY(emit_flagged_rows(ctx, st_p, flag_words, counts, tile_base, o_pr));
        FG_TRY(gather_utf8_begin(ctx, "q8.out_name", person->name, o_pr, out_cap - 16, &g_name, tile_base + st_p.n_tiles));
        FG_HIP(ctx, hipMemcpyAsync(h_off, d_off, sizeof(int64_t) * ((size_t)n_win + 1), hipMemcpyDeviceToHost, ctx->stream));
        FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        offs.assign(h_off, h_off + n_win + 1);
        n_out = offs[n_win];
        gather_utf8_narrow(&g_name, n_out);
    }
    int32_t *o_pid = nullptr;
    FG_TRY(arena_get_t(ctx, "q8.out_p_id", (size_t)n_out + 1, &o_pid));
    FG_TRY(gather_i32(ctx, person->p_id, o_pr, n_out, o_pid));
    FG_TRY(gather_utf8_finish(ctx, g_name, &out->name, &out->name_bytes));
    regime[0] = mode;
    if (mode == 1) {   // a dense call: the next one of this ctx may take the three-launch sequence with these estimates
        fast[0] = n_out + n_out / 8 + 4096;
        fast[1] = out->name_bytes + out->name_bytes / 8 + 65536;
        fast[2] = 1;
    } else {
        fast[2] = 0;
    }
    out->p_id = o_pid;
    out->person_row = o_pr;
    out->win_out_offsets = offs.data();
    out->rows = n_out;
    return FLOCKGPU_OK;
}

}  // extern "C"
