// Delimited text (CSV, '.tbl') -> columns on gfx950: flockgpu_csv_decode.  The semantics are csv.hpp's A-CSV1..7; this file is the device side.
//
//   records : whether a '\n' ends a record depends on the quote state, which no tile of the text knows locally, so the index is count -> summary
//             scan -> emit over 16 KiB tiles with a TWO-STATE summary per tile: (quote parity, terminators if the tile starts outside quotes,
//             terminators if it starts inside).  A lane keeps a 64-bit '"' mask and a 64-bit '\n' mask of its 64 bytes (SWAR compares on 16-byte
//             loads); the prefix XOR of the quote mask is the lane's inside-quotes mask.  One workgroup composes the summaries
//             ((p1, c1) o (p2, c2) = (p1 ^ p2, c1[s] + c2[s ^ p1])) into every tile's true start state and first record number; the emit pass reads
//             the masks only, not the text again.  '""' flips the parity twice, so parity alone indexes well-formed text; what malformed quoting
//             does to it is A-CSV7;
//   parse   : json_parse_kernel's frame -- 256 records per workgroup, their bytes one contiguous range staged in LDS with 16-byte loads, one lane
//             walks one record field by field (csv.hpp: csv_next_field, csv_value).  Numeric columns and their validity bytes are written directly
//             (row = record: coalesced); for a Utf8 field the lane records where the value lies in the INPUT and its length after unquoting.
//             Integers and timestamps of at most 24 bytes reach textnum.hpp as a window of four aligned 64-bit LDS reads.  A workgroup whose
//             records do not fit the stage walks them in global memory: a second instantiation of the same walk, byte-wise windows, correct, not
//             tuned.  The first offender is an atomic minimum over (record, column, code) on a device word that is published with the NULL counts;
//   strings : a column without any '""' is a `take` of byte ranges of the input (gather_utf8 with the (begin, end) pairs as offsets); a column with
//             '""' goes through lengths -> scan -> an unquoting copy, one lane per value.
#include <algorithm>
#include <cstring>

#include "csv.hpp"
#include "gather.hpp"

using namespace flockgpu;

namespace {

constexpr int kCsvMaxFields = 64;
constexpr int kIdxBytes = 64;                     // bytes per lane in the index passes
constexpr int kIdxTile = kBlock * kIdxBytes;      // 16 KiB
constexpr int kParseRecords = kBlock;             // records per workgroup
constexpr int kStageBytes = 48 * 1024;            // most LDS a workgroup stages its records in
constexpr int kInfoWords = 4;                     // {terminators, the last record has no terminator, the text ends inside quotes, -}

struct CsvCol {
    int32_t type, pad;
    void *values;      // numeric: 4 or 8 bytes per row
    uint8_t *valid;    // numeric
    int32_t *pairs;    // Utf8: (begin, end) of the raw value in the input, 2 per row
    int32_t *ulen;     // Utf8: length after unquoting; -(length + 1) where the value holds '""'
};

// ---- record index ------------------------------------------------------------------------------------------------------------------------------
// bit b = byte b of w equals the byte that `pat` repeats (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t eq_mask4(uint32_t w, uint32_t pat) {
    const uint32_t x = w ^ pat;
    const uint32_t t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);   // 0x80 where the byte of x is 0
    return (((t >> 7) * 0x00204081u) >> 21) & 0xFu;
}

// the lane's 64 bytes at p0: *q = '"' mask, *nl = '\n' mask; bytes at or past n read as neither and are not loaded
__device__ __forceinline__ void index_masks(const uint8_t *__restrict__ bytes, int64_t n, int64_t p0, uint64_t *q, uint64_t *nl) {
    uint64_t mq = 0, mn = 0;
    if (p0 + kIdxBytes <= n) {
#pragma unroll
        for (int c = 0; c < kIdxBytes / 16; ++c) {
            const uint4 v = *reinterpret_cast<const uint4 *>(bytes + p0 + c * 16);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                mq |= (uint64_t)eq_mask4(w[i], 0x22222222u) << (c * 16 + i * 4);
                mn |= (uint64_t)eq_mask4(w[i], 0x0A0A0A0Au) << (c * 16 + i * 4);
            }
        }
    } else {
        for (int i = 0; i < kIdxBytes && p0 + i < n; ++i) {
            const uint32_t c = bytes[p0 + i];
            mq |= (uint64_t)(c == (uint32_t)'"') << i;
            mn |= (uint64_t)(c == (uint32_t)'\n') << i;
        }
    }
    *q = mq;
    *nl = mn;
}

// bit i = parity of the set bits of m at or below i
__device__ __forceinline__ uint64_t prefix_xor(uint64_t m) {
    m ^= m << 1;
    m ^= m << 2;
    m ^= m << 4;
    m ^= m << 8;
    m ^= m << 16;
    m ^= m << 32;
    return m;
}

// The lane's inside-quotes mask IF THE TILE STARTS OUTSIDE QUOTES (all 256 lanes call it; s_par: kWavesPerBlock words); *tile_parity = the tile's
__device__ __forceinline__ uint64_t inside_mask(uint64_t q, uint32_t *s_par, uint32_t *tile_parity) {
    const uint32_t par = (uint32_t)__popcll((unsigned long long)q) & 1u;
    const uint64_t b = __ballot(par != 0u);
    const int wave = threadIdx.x >> 6;
    if (lane_id() == 0) s_par[wave] = (uint32_t)__popcll((unsigned long long)b) & 1u;
    __syncthreads();
    uint32_t before = mbcnt(b) & 1u, all = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) {
        before ^= w < wave ? s_par[w] : 0u;
        all ^= s_par[w];
    }
    *tile_parity = all;
    return prefix_xor(q) ^ (before ? ~uint64_t(0) : uint64_t(0));
}

// Pass A: the masks (1/4 of the text: all the emit pass reads) and the tile's summary {parity, terminators if it starts outside, ... inside, 0}
__global__ __launch_bounds__(kBlock) void csv_index_count_kernel(const uint8_t *__restrict__ bytes, int64_t n, uint64_t *__restrict__ q_masks,
                                                                uint64_t *__restrict__ nl_masks, uint4 *__restrict__ summary) {
    __shared__ uint32_t s_par[kWavesPerBlock], s_cnt[kWavesPerBlock];
    const int64_t p0 = (int64_t)blockIdx.x * kIdxTile + (int64_t)threadIdx.x * kIdxBytes;
    uint64_t q, nl;
    index_masks(bytes, n, p0, &q, &nl);
    q_masks[(size_t)blockIdx.x * kBlock + threadIdx.x] = q;
    nl_masks[(size_t)blockIdx.x * kBlock + threadIdx.x] = nl;
    uint32_t parity;
    const uint64_t in = inside_mask(q, s_par, &parity);
    // both counts in one word: at most 16384 terminators per tile
    uint32_t c = (uint32_t)__popcll((unsigned long long)(nl & ~in)) | ((uint32_t)__popcll((unsigned long long)(nl & in)) << 16);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane_id() == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) t += s_cnt[w];
        summary[blockIdx.x] = make_uint4(parity, t & 0xFFFFu, t >> 16, 0u);
    }
}

// The summary scan, ONE workgroup (at most 2^17 tiles): tile_start[t] = {records that end before tile t, tile t starts inside quotes}; info[] as
// kInfoWords says.  It also readies the words the parse pass adds to -- the first-offender word, the NULL counts, the '""' mask -- so that no
// clear is queued for them.
__global__ __launch_bounds__(kBlock) void csv_index_scan_kernel(const uint4 *__restrict__ summary, int32_t tiles, const uint8_t *__restrict__ bytes,
                                                               int64_t n, uint2 *__restrict__ tile_start, uint32_t *__restrict__ info,
                                                               unsigned long long *__restrict__ err, uint32_t *__restrict__ nulls,
                                                               unsigned long long *__restrict__ dq_mask) {
    __shared__ uint32_t s_p[kBlock], s_c0[kBlock], s_c1[kBlock];
    const int32_t chunk = (tiles + kBlock - 1) / kBlock;
    const int32_t t0 = min((int32_t)threadIdx.x * chunk, tiles), t1 = min(t0 + chunk, tiles);
    uint32_t p = 0, c[2] = {0, 0};   // this thread's tiles composed: parity, terminators if the first of them starts outside / inside
    for (int32_t t = t0; t < t1; ++t) {
        const uint4 s = summary[t];
        c[0] += p ? s.z : s.y;
        c[1] += p ? s.y : s.z;
        p ^= s.x;
    }
    s_p[threadIdx.x] = p;
    s_c0[threadIdx.x] = c[0];
    s_c1[threadIdx.x] = c[1];
    __syncthreads();
    if (threadIdx.x == 0) {   // 256 steps: (start state, records before) of every thread's first tile, left in s_p / s_c0
        uint32_t state = 0, base = 0;
        for (int i = 0; i < kBlock; ++i) {
            const uint32_t pi = s_p[i], ci = state ? s_c1[i] : s_c0[i];
            s_p[i] = state;
            s_c0[i] = base;
            state ^= pi;
            base += ci;
        }
        const bool open = state != 0u || n == 0 || bytes[n - 1] != (uint8_t)'\n';
        info[0] = base;
        info[1] = open && n > 0 ? 1u : 0u;
        info[2] = state;
        info[3] = 0u;
        *err = ~0ull;
        *dq_mask = 0ull;
    }
    if (threadIdx.x < kCsvMaxFields) nulls[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t state = s_p[threadIdx.x], base = s_c0[threadIdx.x];
    for (int32_t t = t0; t < t1; ++t) {
        const uint4 s = summary[t];
        tile_start[t] = make_uint2(base, state);
        base += state ? s.z : s.y;
        state ^= s.x;
    }
}

// Pass B: rec_begin[k + 1] = the position after the k-th terminator; rec_begin[0] = 0; an unterminated last record ends at a virtual terminator
// at n (rec_begin[n_rec] = n + 1)
__global__ __launch_bounds__(kBlock) void csv_index_emit_kernel(const uint64_t *__restrict__ q_masks, const uint64_t *__restrict__ nl_masks,
                                                               const uint2 *__restrict__ tile_start, int64_t n, int64_t n_rec, int32_t open_tail,
                                                               int32_t *__restrict__ rec_begin) {
    __shared__ uint32_t s_par[kWavesPerBlock], s_cnt[kWavesPerBlock];
    const int64_t p0 = (int64_t)blockIdx.x * kIdxTile + (int64_t)threadIdx.x * kIdxBytes;
    const uint64_t q = q_masks[(size_t)blockIdx.x * kBlock + threadIdx.x];
    const uint64_t nl = nl_masks[(size_t)blockIdx.x * kBlock + threadIdx.x];
    const uint2 start = tile_start[blockIdx.x];
    uint32_t parity;
    const uint64_t in = inside_mask(q, s_par, &parity) ^ (start.y ? ~uint64_t(0) : uint64_t(0));
    uint64_t m = nl & ~in;
    const uint32_t c = (uint32_t)__popcll((unsigned long long)m);
    const uint32_t incl = wave_incl_scan_u32(c);
    const int wave = threadIdx.x >> 6;
    if (lane_id() == 63) s_cnt[wave] = incl;
    __syncthreads();
    int64_t k = (int64_t)start.x + (incl - c);
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) k += w < wave ? s_cnt[w] : 0u;
    for (; m; m &= m - 1) rec_begin[++k] = (int32_t)(p0 + (__ffsll((unsigned long long)m) - 1) + 1);   // (k + 1 <= the terminators <= n_rec)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        rec_begin[0] = 0;
        if (open_tail) rec_begin[n_rec] = (int32_t)(n + 1);
    }
}

// ---- parse -----------------------------------------------------------------------------------------------------------------------------------------
// The 24-byte window of textnum.hpp whose first byte is s[at], from LDS: four ALIGNED 64-bit reads and a funnel shift (a misaligned LDS read costs 6x on
// gfx950: json.hip).  The caller has made sure that s[at & ~7 .. (at & ~7) + 32) lies inside the stage; what the window holds outside the value is
// whatever the stage holds there, and the parse never looks at it.
__device__ __forceinline__ TextNumWindow lds_window(const uint8_t *s, int32_t at) {
    const uint64_t *q = reinterpret_cast<const uint64_t *>(s + (at & ~7));
    const uint64_t x0 = q[0], x1 = q[1], x2 = q[2], x3 = q[3];
    const int sh = (at & 7) * 8;
    TextNumWindow w;
    w.w[0] = sh ? (x0 >> sh) | (x1 << (64 - sh)) : x0;
    w.w[1] = sh ? (x1 >> sh) | (x2 << (64 - sh)) : x1;
    w.w[2] = sh ? (x2 >> sh) | (x3 << (64 - sh)) : x2;
    return w;
}

// One record, s[p .. e): position x of the text is s[x - off].  kStaged: s is the LDS stage of stage_bytes bytes (integers and timestamps of at most a
// window come from aligned LDS reads); otherwise s is the text in global memory and every value goes through csv.hpp's byte-wise window.
// err: min over ((record number, 0-based with the header) << 16 | column << 8 | code)
template <bool kStaged>
__device__ __forceinline__ void parse_record(const uint8_t *s, int32_t off, int32_t stage_bytes, int32_t p, int32_t e, int64_t row, unsigned long long where,
                                             const CsvCol *__restrict__ cols, int32_t n_fields, uint32_t delim, unsigned long long *err, uint32_t *nulls,
                                             unsigned long long *dq_mask) {
    for (int32_t f = 0; f < n_fields; ++f) {
        CsvField fl;
        uint32_t rc = csv_next_field(s, p, e, delim, &fl);
        const CsvCol col = cols[f];
        if (rc == kCsvOk && col.type != kCsvSkip) {
            if (col.type == kCsvUtf8) {
                col.pairs[2 * row] = fl.begin + off;
                col.pairs[2 * row + 1] = fl.end + off;
                col.ulen[row] = fl.dq ? -(fl.ulen + 1) : fl.ulen;
                if (fl.dq) atomicOr(dq_mask, 1ull << f);
            } else {
                uint64_t bits = 0;
                const int32_t len = fl.end - fl.begin;
                const bool null = len == 0;
                if (!null) {
                    const bool is_int = col.type == kCsvInt32 || col.type == kCsvInt64 || col.type == kCsvUInt64;
                    if (kStaged && is_int && len <= kTextNumWindow && fl.end >= kTextNumWindow) {          // right-aligned: the window ends where the value ends
                        const TextNumKind kind = col.type == kCsvInt32 ? TextNumKind::I32 : col.type == kCsvInt64 ? TextNumKind::I64 : TextNumKind::U64;
                        rc = textnum_int(kind, lds_window(s, fl.end - kTextNumWindow), len, &bits) ? kCsvOk : kCsvErrValue;
                    } else if (kStaged && col.type == kCsvTimestampMs && len < kTextNumWindow && (fl.begin & ~7) + 32 <= stage_bytes) {   // left-aligned
                        int64_t ms = 0;
                        rc = textnum_ts(lds_window(s, fl.begin), len, &ms) ? kCsvOk : kCsvErrValue;
                        bits = (uint64_t)ms;
                    } else {
                        rc = csv_value(col.type, s + fl.begin, len, &bits);
                    }
                }
                if (col.type == kCsvInt32) static_cast<int32_t *>(col.values)[row] = (int32_t)bits;
                else static_cast<uint64_t *>(col.values)[row] = bits;
                col.valid[row] = null ? 0 : 1;
                if (null) atomicAdd(nulls + f, 1u);
            }
        }
        if (rc == kCsvOk && f + 1 < n_fields && fl.next >= e) {
            rc = kCsvErrFewFields;
        } else if (rc == kCsvOk && f + 1 == n_fields && fl.next < e) {
            rc = kCsvErrManyFields;
        }
        if (rc != kCsvOk) {
            atomicMin(err, where | ((unsigned long long)f << 8) | rc);
            return;
        }
        p = fl.next + 1;
    }
}

__global__ __launch_bounds__(kBlock) void csv_parse_kernel(const uint8_t *__restrict__ bytes, int64_t n_bytes, const int32_t *__restrict__ rec_begin,
                                                          int64_t n_rows, int32_t header, const CsvCol *__restrict__ cols, int32_t n_fields,
                                                          uint32_t delim, int32_t stage_bytes, unsigned long long *err, uint32_t *nulls,
                                                          unsigned long long *dq_mask) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_stage[];   // stage_bytes of dynamic LDS
    const int32_t *__restrict__ rec = rec_begin + header;
    const int64_t r0 = (int64_t)blockIdx.x * kParseRecords;
    const int64_t r1 = min(r0 + kParseRecords, n_rows);
    const int32_t b0 = rec[r0], b1 = (int32_t)min((int64_t)rec[r1], n_bytes);
    const int32_t a0 = b0 & ~15;
    const bool staged = b1 - a0 + 16 <= stage_bytes;   // block-uniform; 16 bytes to spare: a window's aligned reads run past the value by up to 8
    const int64_t row = r0 + threadIdx.x;
    const int64_t row_c = min(row, n_rows - 1);
    const int32_t begin = rec[row_c], term = rec[row_c + 1] - 1;   // asked for before the staging so that the loads overlap it
    if (staged) {
        for (int32_t o = a0 + (int32_t)threadIdx.x * 16; o < b1; o += kBlock * 16) {
            if ((int64_t)o + 16 <= n_bytes) {
                *reinterpret_cast<uint4 *>(s_stage + (o - a0)) = *reinterpret_cast<const uint4 *>(bytes + o);
            } else {
                for (int32_t i = o; i < b1; ++i) s_stage[i - a0] = bytes[i];
            }
        }
    }
    __syncthreads();
    if (row >= n_rows) return;
    const int32_t off = staged ? a0 : 0;
    int32_t p = begin - off, e = term - off;
    const unsigned long long where = (unsigned long long)(row + header) << 16;
    // '\r\n'; in front of the virtual terminator of an unterminated last record a '\r' is a bare one
    if ((int64_t)term < n_bytes && e > p && (staged ? s_stage[e - 1] : bytes[e - 1]) == (uint8_t)'\r') --e;
    if (p >= e) {
        atomicMin(err, where | kCsvErrBlank);
        return;
    }
    if (staged) parse_record<true>(s_stage, off, stage_bytes, p, e, row, where, cols, n_fields, delim, err, nulls, dq_mask);
    else parse_record<false>(bytes, 0, 0, p, e, row, where, cols, n_fields, delim, err, nulls, dq_mask);
}

// ---- Utf8 after the parse ----------------------------------------------------------------------------------------------------------------------------
// len[i + 1] = the unquoted length of value i (the scan turns them into offsets)
__global__ __launch_bounds__(kBlock) void csv_string_lengths_kernel(const int32_t *__restrict__ ulen, int64_t n, int32_t *__restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        const int32_t u = ulen[i];
        len[i + 1] = u < 0 ? -(u + 1) : u;
    }
    if (i == 0) len[0] = 0;
}

// the unquoting copy of a column that holds '""': one lane per value (offsets already scanned)
__global__ __launch_bounds__(kBlock) void csv_unquote_kernel(const uint8_t *__restrict__ bytes, const int32_t *__restrict__ pairs,
                                                            const int32_t *__restrict__ off, int64_t n, uint8_t *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    csv_unquote(bytes, pairs[2 * i], pairs[2 * i + 1], dst + off[i]);
}

__global__ __launch_bounds__(kBlock) void csv_even_rows_kernel(int32_t *__restrict__ rows, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) rows[i] = (int32_t)(2 * i);
}

const char *type_name(int32_t t) {
    static const char *names[] = {"Int32", "Int64", "UInt64", "Float64", "Timestamp(ms)", "Utf8"};
    return t >= 0 && t <= kCsvUtf8 ? names[t] : "skipped";
}

}  // namespace

extern "C" {

int flockgpu_csv_decode(flockgpu_ctx *ctx, const uint8_t *text, int64_t n_bytes, const flockgpu_csv_field *fields, int32_t n_fields,
                        const flockgpu_csv_options *opt, flockgpu_csv_column *out, int64_t *rows) {
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    if (!fields || !opt || !out || !rows || n_bytes < 0 || n_fields < 1 || (n_bytes > 0 && !text)) return fail(ctx, FLOCKGPU_ERR_INVALID, "csv: null argument");
    if (n_fields > kCsvMaxFields) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "csv: more than %d columns", kCsvMaxFields);
    if (n_bytes >= (int64_t(1) << 31) - 16) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "csv: at most 2^31 bytes of text per call (Arrow Utf8 offsets are int32)");
    if (reinterpret_cast<uintptr_t>(text) & 15) return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "csv: the text must be 16-byte aligned");
    const uint32_t delim = opt->delimiter;
    if (delim >= 0x80u || delim == (uint32_t)'"' || delim == (uint32_t)'\r' || delim == (uint32_t)'\n')
        return fail(ctx, FLOCKGPU_ERR_INVALID, "csv: the delimiter is an ASCII byte other than '\"', CR and LF (got 0x%02x)", delim);
    for (int f = 0; f < n_fields; ++f)
        if (fields[f].type < kCsvSkip || fields[f].type > kCsvUtf8) return fail(ctx, FLOCKGPU_ERR_INVALID, "csv: column %d: unknown type %d", f, fields[f].type);
    const int32_t header = opt->has_header ? 1 : 0;
    FG_HIP(ctx, hipSetDevice(ctx->device));
    for (int f = 0; f < n_fields; ++f)
        if (fields[f].type != kCsvSkip) out[f] = flockgpu_csv_column{};
    *rows = 0;

    // ---- record index
    const int64_t tiles = div_up(std::max<int64_t>(n_bytes, 1), kIdxTile);
    uint64_t *q_masks = nullptr, *nl_masks = nullptr;
    uint4 *summary = nullptr;
    uint2 *tile_start = nullptr;
    uint32_t *d_info = nullptr, *h_info = nullptr, *d_nulls = nullptr, *h_nulls = nullptr;
    unsigned long long *d_err = nullptr, *h_err = nullptr;   // [0] the first offender, [1] the columns that hold '""'
    FG_TRY(arena_get_t(ctx, "csv.q_masks", (size_t)tiles * kBlock, &q_masks));
    FG_TRY(arena_get_t(ctx, "csv.nl_masks", (size_t)tiles * kBlock, &nl_masks));
    FG_TRY(arena_get_t(ctx, "csv.summary", (size_t)tiles, &summary));
    FG_TRY(arena_get_t(ctx, "csv.tile_start", (size_t)tiles, &tile_start));
    FG_TRY(arena_get_t(ctx, "csv.info", kInfoWords, &d_info));
    FG_TRY(pinned_get_t(ctx, "csv.info", kInfoWords, &h_info));
    FG_TRY(arena_get_t(ctx, "csv.nulls", kCsvMaxFields, &d_nulls));
    FG_TRY(pinned_get_t(ctx, "csv.nulls", kCsvMaxFields, &h_nulls));
    FG_TRY(arena_get_t(ctx, "csv.err", 2, &d_err));
    FG_TRY(pinned_get_t(ctx, "csv.err", 2, &h_err));
    int64_t n_rec = 0;
    bool open_tail = false;
    if (n_bytes > 0) {
        {
            LaunchScope ls(ctx, "csv_index_count_kernel");
            hipLaunchKernelGGL(csv_index_count_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, ctx->stream, text, n_bytes, q_masks, nl_masks, summary);
        }
        FG_TRY(check_launch(ctx, "csv_index_count_kernel"));
        {
            LaunchScope ls(ctx, "csv_index_scan_kernel");
            hipLaunchKernelGGL(csv_index_scan_kernel, dim3(1), dim3(kBlock), 0, ctx->stream, summary, (int32_t)tiles, text, n_bytes, tile_start, d_info, d_err,
                               d_nulls, d_err + 1);
        }
        FG_TRY(check_launch(ctx, "csv_index_scan_kernel"));
        FG_TRY(publish_words(ctx, PublishList().add(h_info, d_info, kInfoWords)));
        FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        open_tail = h_info[1] != 0;
        n_rec = (int64_t)h_info[0] + (open_tail ? 1 : 0);
    }
    const int64_t n_rows = std::max<int64_t>(n_rec - header, 0);
    int32_t *rec_begin = nullptr;
    FG_TRY(arena_get_t(ctx, "csv.rec_begin", (size_t)n_rec + 2, &rec_begin));
    if (n_bytes > 0) {
        LaunchScope ls(ctx, "csv_index_emit_kernel");
        hipLaunchKernelGGL(csv_index_emit_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, ctx->stream, q_masks, nl_masks, tile_start, n_bytes, n_rec,
                           open_tail ? 1 : 0, rec_begin);
    }
    FG_TRY(check_launch(ctx, "csv_index_emit_kernel"));

    // ---- parse
    CsvCol *d_cols = nullptr, *h_cols = nullptr;
    FG_TRY(arena_get_t(ctx, "csv.cols", kCsvMaxFields, &d_cols));
    FG_TRY(pinned_get_t(ctx, "csv.cols", kCsvMaxFields, &h_cols));
    int32_t *soff[kCsvMaxFields] = {};
    std::vector<CsvCol> cols((size_t)n_fields);
    for (int f = 0; f < n_fields; ++f) {
        char name[48];
        CsvCol &c = cols[(size_t)f];
        c = CsvCol{};
        c.type = fields[f].type;
        if (c.type == kCsvSkip) continue;
        if (c.type == kCsvUtf8) {
            snprintf(name, sizeof name, "csv.pairs.%d", f);
            FG_TRY(arena_get_t(ctx, name, (size_t)2 * n_rows + 4, &c.pairs));
            snprintf(name, sizeof name, "csv.ulen.%d", f);
            FG_TRY(arena_get_t(ctx, name, (size_t)n_rows + 4, &c.ulen));
            snprintf(name, sizeof name, "csv.str_off.%d", f);
            FG_TRY(arena_get_t(ctx, name, (size_t)n_rows + 4, &soff[f]));
        } else {
            snprintf(name, sizeof name, "csv.values.%d", f);
            FG_TRY(arena_get(ctx, name, ((size_t)n_rows + 4) * (c.type == kCsvInt32 ? 4 : 8), &c.values));
            snprintf(name, sizeof name, "csv.valid.%d", f);
            FG_TRY(arena_get_t(ctx, name, (size_t)n_rows + 16, &c.valid));
        }
    }
    h_err[0] = ~0ull;
    h_err[1] = 0;
    std::memset(h_nulls, 0, sizeof(uint32_t) * kCsvMaxFields);
    if (n_rows > 0) {
        std::memcpy(h_cols, cols.data(), sizeof(CsvCol) * (size_t)n_fields);   // (the stream is idle: the wait above)
        FG_HIP(ctx, hipMemcpyAsync(d_cols, h_cols, sizeof(CsvCol) * (size_t)n_fields, hipMemcpyHostToDevice, ctx->stream));
        // LDS per workgroup follows the text, as the JSON parse does: 1.25 x the average bytes of 256 records
        const int64_t want = (n_bytes / n_rec + 1) * kParseRecords * 5 / 4 + 64;
        const int32_t stage_bytes = (int32_t)std::min<int64_t>(kStageBytes, (want + 1023) & ~int64_t(1023));
        {
            LaunchScope ls(ctx, "csv_parse_kernel");
            hipLaunchKernelGGL(csv_parse_kernel, dim3((unsigned)div_up(n_rows, kParseRecords)), dim3(kBlock), (size_t)stage_bytes, ctx->stream, text, n_bytes,
                               rec_begin, n_rows, header, d_cols, n_fields, delim, stage_bytes, d_err, d_nulls, d_err + 1);
        }
        FG_TRY(check_launch(ctx, "csv_parse_kernel"));
        for (int f = 0; f < n_fields; ++f) {
            if (cols[(size_t)f].type != kCsvUtf8) continue;
            hipLaunchKernelGGL(csv_string_lengths_kernel, dim3((unsigned)div_up(n_rows, kBlock)), dim3(kBlock), 0, ctx->stream, cols[(size_t)f].ulen, n_rows, soff[f]);
            FG_TRY(check_launch(ctx, "csv_string_lengths_kernel"));
        }
        // the error word rides with the NULL counts: one launch and one wait, whether or not a record failed
        FG_TRY(publish_words(ctx, PublishList().add(h_err, d_err, 4).add(h_nulls, d_nulls, kCsvMaxFields)));
        FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (h_err[0] != ~0ull) {
        const long long record = (long long)(h_err[0] >> 16) + 1;
        const int col = (int)((h_err[0] >> 8) & 0xFF);
        const uint32_t code = (uint32_t)(h_err[0] & 0xFF);
        const char *tn = type_name(col < n_fields ? fields[col].type : kCsvSkip);
        switch (code) {
        case kCsvErrBlank: return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "csv: record %lld: blank line", record);
        case kCsvErrBareCr: return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "csv: record %lld: column %d: a bare CR outside quotes", record, col);
        case kCsvErrStrayQuote: return fail(ctx, FLOCKGPU_ERR_INVALID, "csv: record %lld: column %d: a quote inside an unquoted field", record, col);
        case kCsvErrAfterQuote: return fail(ctx, FLOCKGPU_ERR_INVALID, "csv: record %lld: column %d: bytes between the closing quote and the delimiter", record, col);
        case kCsvErrOpenQuote: return fail(ctx, FLOCKGPU_ERR_INVALID, "csv: record %lld: column %d: unterminated quote", record, col);
        case kCsvErrFewFields: return fail(ctx, FLOCKGPU_ERR_INVALID, "csv: record %lld: %d fields where %d are declared", record, col + 1, n_fields);
        case kCsvErrManyFields: return fail(ctx, FLOCKGPU_ERR_INVALID, "csv: record %lld: more than the %d declared fields", record, n_fields);
        case kCsvErrFloat:
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "csv: record %lld: column %d: not a Float64 inside the exactly converted range (significand <= 2^53, exponent in [-22, 22])",
                        record, col);
        default: return fail(ctx, FLOCKGPU_ERR_INVALID, "csv: record %lld: column %d: the value does not parse as %s", record, col, tn);
        }
    }

    // ---- Utf8
    int32_t *even = nullptr;
    for (int f = 0; f < n_fields; ++f) {
        const CsvCol &c = cols[(size_t)f];
        if (c.type == kCsvSkip) continue;
        if (c.type != kCsvUtf8) {
            out[f].values = c.values;
            out[f].valid = c.valid;
            out[f].null_count = h_nulls[f];
            continue;
        }
        char name[48];
        if (!((h_err[1] >> f) & 1ull)) {   // a plain take of byte ranges of the input
            if (!even) {
                FG_TRY(arena_get_t(ctx, "csv.even_rows", (size_t)n_rows + 4, &even));
                if (n_rows > 0) {
                    hipLaunchKernelGGL(csv_even_rows_kernel, dim3((unsigned)div_up(n_rows, kBlock)), dim3(kBlock), 0, ctx->stream, even, n_rows);
                    FG_TRY(check_launch(ctx, "csv_even_rows_kernel"));
                }
            }
            snprintf(name, sizeof name, "csv.utf8.%d", f);
            flockgpu_utf8 src{c.pairs, text};
            FG_TRY(gather_utf8(ctx, name, src, even, n_rows, &out[f].utf8, &out[f].utf8_bytes));
        } else {
            FG_TRY(inclusive_scan_i32(ctx, "csv.str_scan", soff[f], n_rows + 1));
            uint32_t *h_tot = nullptr;
            FG_TRY(pinned_get_t(ctx, "csv.str_total", 1, &h_tot));
            FG_TRY(publish_words(ctx, PublishList().add(h_tot, soff[f] + n_rows, 1)));
            FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
            uint8_t *dst = nullptr;
            snprintf(name, sizeof name, "csv.str_bytes.%d", f);
            FG_TRY(arena_get_t(ctx, name, (size_t)*h_tot + 16, &dst));
            {
                LaunchScope ls(ctx, "csv_unquote_kernel");
                hipLaunchKernelGGL(csv_unquote_kernel, dim3((unsigned)div_up(n_rows, kBlock)), dim3(kBlock), 0, ctx->stream, text, c.pairs, soff[f], n_rows, dst);
            }
            FG_TRY(check_launch(ctx, "csv_unquote_kernel"));
            out[f].utf8.offsets = soff[f];
            out[f].utf8.data = dst;
            out[f].utf8_bytes = *h_tot;
        }
    }
    *rows = n_rows;
    return FLOCKGPU_OK;
}

}  // extern "C"
