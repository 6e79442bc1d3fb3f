// COUNT(DISTINCT x) per group (distinct.hpp): one streaming pass over (group id, argument) into a global open-addressing set.
#include "distinct.hpp"

#include <algorithm>

#include "hashtab.hpp"

using namespace flockgpu;

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

inline unsigned grid_for(flockgpu_ctx *ctx, int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(div_up(n, kBlock), (int64_t)ctx->num_cus * 16));
}
inline uint64_t pow2_at_least(uint64_t v) {
    uint64_t c = 1024;
    while (c < v) c <<= 1;
    return c;
}

// the call's scalars: [0] error word (probing was cut off: the table is too small -- or a group id lies outside the counts), [1] claimed slots = distinct (group, value) pairs
constexpr int kStatWords = 2;

// table = empty, counts = 0, stat = 0: one launch
__global__ __launch_bounds__(kBlock) void distinct_init_kernel(uint64_t *__restrict__ table, int64_t cap, uint64_t *__restrict__ counts, int64_t n_groups,
                                                               uint32_t *__restrict__ stat) {
    const int64_t n = cap > n_groups ? cap : n_groups;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        if (i < cap) table[i] = kEmpty64;
        if (i < n_groups) counts[i] = 0;
        if (i < kStatWords) stat[i] = 0;
    }
}

template <bool kI32>
__device__ __forceinline__ uint64_t arg_bits(const void *__restrict__ v, int64_t i) {
    if (kI32) return (uint64_t)(int64_t) static_cast<const int32_t *>(v)[i];   // (sign-extended: equal values, equal bits)
    return static_cast<const uint64_t *>(v)[i];
}

// One lane per row.  kGrouped: gid[i] names the row's group and the claiming row adds 1 to counts[gid] (at most one add per distinct pair); else every
// row is in group 0 and the claims are summed per workgroup first -- every row its own value would be one add per row to ONE word otherwise.
template <bool kI32, bool kGrouped>
__global__ __launch_bounds__(kBlock) void distinct_insert_kernel(const int32_t *__restrict__ gid, const void *__restrict__ values, const uint8_t *__restrict__ valid,
                                                                 int64_t n, int64_t n_groups, uint64_t *table, uint64_t cap, unsigned long long *counts,
                                                                 uint32_t *stat) {
    __shared__ uint64_t s_claims[kWavesPerBlock];
    const uint32_t limit = cap < (uint64_t)kMaxProbe ? (uint32_t)cap : kMaxProbe;
    uint64_t claims = 0;
    bool cut = false;
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += (int64_t)gridDim.x * kBlock) {   // (block-uniform: every lane of a wave takes every turn)
        const int64_t i = base + threadIdx.x;
        bool live = i < n && (!valid || valid[i]);   // NULL arguments are skipped (A-D1)
        uint64_t v = 0;
        int32_t g = 0;
        if (live) {
            v = arg_bits<kI32>(values, i);
            g = kGrouped ? gid[i] : 0;
            if (kGrouped && (uint64_t)(uint32_t)g >= (uint64_t)n_groups) {   // (an id outside the counts: nothing is written for it, the call fails)
                cut = true;
                live = false;
            }
        }
        // The wave's first live row speaks for every lane that holds the same pair: under NEXMark's skew (three bids in four from one bidder, one in two
        // on one auction) most of a wave would read ONE slot, and the L2 channel that owns it serves a request per wave, not per pair.
        const unsigned long long live_mask = __ballot(live);
        if (live_mask) {
            const int lead = __ffsll(live_mask) - 1;
            const uint64_t lead_v = __shfl(v, lead, 64);
            const int32_t lead_g = __shfl(g, lead, 64);
            if ((int)(threadIdx.x & 63) != lead && lead_v == v && lead_g == g) live = false;
        }
        if (live) {
            const uint64_t h = mix64(v + (uint64_t)(uint32_t)g * 0x9E3779B97F4A7C15ull);
            const uint64_t tag = h >> 32, mine = (tag << 32) | (uint32_t)i;   // (rows stay below 2^30: no slot holds kEmpty64)
            uint64_t s = h & (cap - 1);
            bool done = false;
#pragma unroll 1
            for (uint32_t probe = 0; probe < limit; ++probe) {
                uint64_t cur = ld64(&table[s]);
                if (cur == kEmpty64) {
                    if (cas64(&table[s], cur, mine)) {   // (a failed exchange leaves the winner's word in `cur`)
                        ++claims;
                        if (kGrouped) __hip_atomic_fetch_add(&counts[g], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        done = true;
                        break;
                    }
                }
                if ((cur >> 32) == tag) {
                    // the slot's first row: its group and value are read from the input columns, which this launch does not write
                    const int64_t f = (int64_t)(uint32_t)cur;
                    if ((kGrouped ? gid[f] : 0) == g && arg_bits<kI32>(values, f) == v) {
                        done = true;
                        break;
                    }
                }
                s = (s + 1) & (cap - 1);
            }
            cut = cut || !done;
        }
    }
    if (cut) __hip_atomic_store(&stat[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    claims = wave_sum_u64(claims);
    if ((threadIdx.x & 63) == 0) s_claims[threadIdx.x >> 6] = claims;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t total = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) total += s_claims[w];
        if (total) {
            __hip_atomic_fetch_add(&stat[1], (uint32_t)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!kGrouped) __hip_atomic_fetch_add(&counts[0], (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

namespace flockgpu {

int distinct_count_by_group(flockgpu_ctx *ctx, const char *name, const int32_t *gid, int64_t n_groups, const DevColumn &arg, int64_t rows, uint64_t *counts) {
    const std::string base = name;
    if (n_groups < 0 || (!gid && n_groups != 1) || !counts) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: distinct count without groups or a place for its counts", name);
    if (arg.type == ColType::F64) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: distinct_count needs an integer or Utf8 column", name);
    if (rows < 0) rows = 0;
    if (rows >= (int64_t(1) << 30)) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: more than 2^30 rows in a distinct count", name);
    if (arg.all_null) rows = 0;   // nothing but NULLs: every count is 0
    const void *values = arg.values;
    bool i32 = arg.type == ColType::I32;
    if (arg.type == ColType::UTF8 && rows > 0) {   // equal strings, equal codes: the same pass over the codes (a NULL's code is never read)
        int64_t *codes = nullptr;
        FG_TRY(arena_get_t(ctx, (base + ".codes").c_str(), (size_t)rows + 2, &codes));
        FG_TRY(utf8_codes(ctx, (base + ".dict").c_str(), arg, rows, codes, nullptr, 0, nullptr));
        values = codes;
        i32 = false;
    }
    if (rows > 0 && !values) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: distinct count over a column that was not materialised", name);
    // The table: two slots per row always hold.  A name that has been here before is sized for three slots per distinct pair it had then (a
    // streaming host sends window after window of one shape; NEXMark's bids repeat their bidders and auctions many times over).
    const uint64_t full = pow2_at_least((uint64_t)std::max<int64_t>(rows, 1) * 2);
    std::vector<int64_t> &hint = ctx->host_i64[base + ".pairs_hint"];   // {distinct pairs of the last call under this name + 1}
    uint64_t cap = hint.empty() || hint[0] <= 0 ? full : std::min(full, pow2_at_least((uint64_t)std::max<int64_t>((hint[0] - 1) * 3, 1024)));
    uint64_t *table = nullptr;
    uint32_t *d_stat = nullptr, *h_stat = nullptr;
    FG_TRY(arena_get_t(ctx, (base + ".stat").c_str(), 4, &d_stat));
    FG_TRY(pinned_get_t(ctx, (base + ".stat").c_str(), 4, &h_stat));
    for (;;) {
        if (rows == 0) cap = 0;   // (counts alone are cleared)
        if (cap) FG_TRY(arena_get_t(ctx, (base + ".table").c_str(), (size_t)cap, &table));
        {
            LaunchScope ls(ctx, "distinct_init_kernel");
            hipLaunchKernelGGL(distinct_init_kernel, dim3(grid_for(ctx, std::max<int64_t>((int64_t)cap, std::max<int64_t>(n_groups, kStatWords)))), dim3(kBlock), 0,
                               ctx->stream, table, (int64_t)cap, counts, n_groups, d_stat);
        }
        FG_TRY(check_launch(ctx, "distinct_init_kernel"));
        if (rows == 0) return FLOCKGPU_OK;
        {
            LaunchScope ls(ctx, "distinct_insert_kernel");
            const dim3 grid(grid_for(ctx, rows)), block(kBlock);
            unsigned long long *c = reinterpret_cast<unsigned long long *>(counts);
            if (gid) {
                if (i32) hipLaunchKernelGGL((distinct_insert_kernel<true, true>), grid, block, 0, ctx->stream, gid, values, arg.valid, rows, n_groups, table, cap, c, d_stat);
                else hipLaunchKernelGGL((distinct_insert_kernel<false, true>), grid, block, 0, ctx->stream, gid, values, arg.valid, rows, n_groups, table, cap, c, d_stat);
            } else {
                if (i32) hipLaunchKernelGGL((distinct_insert_kernel<true, false>), grid, block, 0, ctx->stream, gid, values, arg.valid, rows, n_groups, table, cap, c, d_stat);
                else hipLaunchKernelGGL((distinct_insert_kernel<false, false>), grid, block, 0, ctx->stream, gid, values, arg.valid, rows, n_groups, table, cap, c, d_stat);
            }
        }
        FG_TRY(check_launch(ctx, "distinct_insert_kernel"));
        pinned_pending32(h_stat, kStatWords);
        FG_TRY(publish_words(ctx, PublishList().add(h_stat, d_stat, kStatWords)));
        FG_TRY(wait_pinned32(ctx, h_stat, kStatWords));
        if (!h_stat[0]) break;
        if (cap >= full) return fail(ctx, FLOCKGPU_ERR_CAPACITY, "%s: distinct table overflow", name);
        cap = full;   // the hint was wrong: ONE more pass over a table that always holds
    }
    hint.assign(1, (int64_t)h_stat[1] + 1);
    return FLOCKGPU_OK;
}

}  // namespace flockgpu
