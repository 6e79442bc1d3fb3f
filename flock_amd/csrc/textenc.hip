// Columns -> JSON lines / delimited text on gfx950: flockgpu_json_lines_encode, flockgpu_csv_encode.  The rules are textenc.hpp's A-ENC1..10; this file is
// the device side.  A column table goes to the device once per call: type, pointers, and the bytes in front of the value ('{"name":' / ',"name":' for
// JSON, nothing / the delimiter for CSV) as little-endian words.
//   class  : one launch per Utf8 column, utf8_chars_kernel's streaming shape (strlen.hip): a workgroup takes 2048 rows and streams the byte range they
//            span in rounds of 32 KiB, every 16 bytes with one aligned load (the partial first and last chunk byte by byte: nothing outside the rows is
//            read); a lane reduces its chunk to TWO 16-bit class masks (JSON: escaped bytes, \u00xx bytes; CSV: '"', bytes that force quotes) that are
//            staged in LDS, then a lane takes rows and counts the bits inside [begin, end).  Out: the row's extra bytes, and per column one word that
//            says whether any class byte was seen: where it is 0 the later passes do not read the extras and copy every value verbatim;
//   length : one lane per row walks the column table: constant bytes + digit counts + Utf8 lengths and extras; the CSV timestamp range check (the first
//            offender is an atomic minimum over (row, column) on a device word; a word of PINNED memory is stored to only on failure and read after the
//            wait for the byte total, which the call has anyway).  Per row the length, per wave the sum for the tile scan (scan.hpp);
//   emit   : a workgroup takes kEncTile consecutive rows, whose output is one contiguous range.  It assembles the range in an LDS stage in rounds of
//            kEncStage bytes and leaves as aligned 16-byte non-temporal stores; only the partial chunk at each end of the tile's range goes byte by byte,
//            its neighbour owns the rest.  One lane walks one row, and the workgroup sweeps the columns together: the SAME column in every lane, so the
//            table arrives in scalar registers and the type switch is uniform.  A column whose bytes lie inside the round -- all but the ones on a
//            round's seam -- takes the straight path: the constant bytes in front (uniform words, a funnel shift by the lane's q & 3) and the numbers
//            (formatted in registers: numtext.hpp numtext_place) land as ALIGNED dwords, their ends byte by byte; text is read in aligned dwords that
//            lie inside the value and goes out whole where no class byte is in them, through the escape otherwise.  On a seam the same walk runs as a
//            resumable cursor (column, part, source byte) whose stores are clipped to the round; an element that crosses the seam is written again,
//            clipped, by the next round.  A value or a row larger than the stage is therefore correct -- one lane per row, a source byte at a time:
//            not tuned.
// Every row index is checked against `rows`; a tile writes output bytes [tile_base, tile_base + tile bytes) only.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gather.hpp"
#include "scan.hpp"
#include "textenc.hpp"

using namespace flockgpu;

namespace {

constexpr int kEncTile = kBlock;            // rows of an emit workgroup: one lane per row
constexpr int kEncStage = 32 * 1024;        // bytes of the LDS stage = of a round
constexpr int kClsRows = 2048;              // rows of a class-pass workgroup
constexpr int kClsRoundBytes = 32768;
constexpr int kClsChunks = kClsRoundBytes / 16;
constexpr uint64_t kLenCap = uint64_t(1) << 31;   // a row's / a wave's length saturates here: the call is refused anyway

struct EncCol {
    const void *values;        // Int32: 4 bytes per row; the other numbers: 8
    const uint8_t *valid;      // or null
    const int32_t *off;        // Utf8
    const uint8_t *bytes;      // Utf8
    const int32_t *extra;      // Utf8: the class pass's per-row result
    const uint32_t *any;       // Utf8: 0 = the column holds no class byte at all
    int32_t type, pre_len;
    uint32_t pre[kTextEncPreWords];   // the bytes in front of the value, in memory order
};

// ---- class pass --------------------------------------------------------------------------------------------------------------------------------------
template <TextFormat F>
__global__ __launch_bounds__(kBlock) void textenc_class_kernel(const int32_t *__restrict__ off, const uint8_t *__restrict__ bytes, int64_t n_rows, uint32_t delim,
                                                               int32_t *__restrict__ extra, uint32_t *__restrict__ any) {
    __shared__ __attribute__((aligned(16))) uint16_t s_a[kClsChunks + 4], s_b[kClsChunks + 4];   // (+ 4: the last word read whole)
    __shared__ int32_t s_off[kClsRows + 1];
    __shared__ uint32_t s_cnt[kClsRows];   // JSON: the extra bytes so far; CSV: (the '"' so far) << 1 | a special byte seen
    __shared__ uint32_t s_any;
    const int tid = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kClsRows;
    const int32_t nr = (int32_t)(row0 >= n_rows ? 0 : (n_rows - row0 < kClsRows ? n_rows - row0 : kClsRows));
    if (nr <= 0) return;   // (block-uniform)
    for (int i = tid; i <= nr; i += kBlock) s_off[i] = off[row0 + i];
    for (int i = tid; i < nr; i += kBlock) s_cnt[i] = 0;
    if (tid < 4) s_a[kClsChunks + tid] = s_b[kClsChunks + tid] = 0;
    if (tid == 0) s_any = 0;
    __syncthreads();
    const int64_t B0 = s_off[0], B1 = s_off[nr];
    const uint64_t *a64 = reinterpret_cast<const uint64_t *>(s_a), *b64 = reinterpret_cast<const uint64_t *>(s_b);
    // u = byte offset + mis: the coordinate in which 16-byte-aligned ADDRESSES are multiples of 16
    const int64_t mis = (int64_t)(reinterpret_cast<uintptr_t>(bytes) & 15u);
    bool seen = false;
    for (int64_t G = (B0 + mis) & ~int64_t(15); G - mis < B1; G += kClsRoundBytes) {
        const int64_t base = G - mis;   // byte offset of the round's position 0
        uint32_t ma[kClsChunks / kBlock], mb[kClsChunks / kBlock];
#pragma unroll
        for (int i = 0; i < kClsChunks / kBlock; ++i) {
            const int64_t o = base + (int64_t)(i * kBlock + tid) * 16;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            uint32_t live = 0xffffu;   // the chunk's bytes that are the rows'
            if (o >= B0 && o + 16 <= B1) {
                v = stream_load4u(reinterpret_cast<const uint32_t *>(bytes + o));   // (read once here; the emit pass reads the bytes again)
            } else if (o + 16 > B0 && o < B1) {   // the first / last, partial chunk of the workgroup's bytes: byte by byte, nothing outside them is touched
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                live = 0;
                for (int k = 0; k < 16; ++k)
                    if (o + k >= B0 && o + k < B1) {
                        w[k >> 2] |= (uint32_t)bytes[o + k] << (8 * (k & 3));
                        live |= 1u << k;
                    }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
                live = 0;
            }
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            uint32_t a = 0, b = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t x, y;
                if (F == TextFormat::Json) textenc::json_class4(w[k], &x, &y);
                else textenc::csv_class4(w[k], delim, &x, &y);
                a |= x << (4 * k);
                b |= y << (4 * k);
            }
            ma[i] = a & live;   // (a byte that was not loaded reads as 0x00, a JSON class byte: masked)
            mb[i] = b & live;
            seen = seen || ((ma[i] | mb[i]) != 0u);
        }
        __syncthreads();   // the previous round's counts are taken
#pragma unroll
        for (int i = 0; i < kClsChunks / kBlock; ++i) {
            s_a[i * kBlock + tid] = (uint16_t)ma[i];
            s_b[i * kBlock + tid] = (uint16_t)mb[i];
        }
        __syncthreads();
        for (int r = tid; r < nr; r += kBlock) {
            int64_t a = (int64_t)s_off[r] - base, b = (int64_t)s_off[r + 1] - base;   // the row's positions in this round: [a, b)
            a = a < 0 ? 0 : a;
            b = b > kClsRoundBytes ? kClsRoundBytes : b;
            if (a >= b) continue;
            uint32_t ca = 0, cb = 0;
            for (int w = (int)(a >> 6); w <= (int)((b - 1) >> 6); ++w) {
                const int64_t lo = (int64_t)w << 6;
                ca += (uint32_t)slicebits::popcount64(slicebits::clip_word(a64[w], lo, a, b));
                cb += (uint32_t)slicebits::popcount64(slicebits::clip_word(b64[w], lo, a, b));
            }
            if (F == TextFormat::Json) s_cnt[r] += textenc::json_extra_of(ca, cb);
            else s_cnt[r] = (((s_cnt[r] >> 1) + ca) << 1) | (s_cnt[r] & 1u) | (cb ? 1u : 0u);
        }
    }
    if (seen) s_any = 1u;   // (every lane that stores stores the same word)
    __syncthreads();
    for (int i = tid; i < nr; i += kBlock) {
        const uint32_t c = s_cnt[i];
        extra[row0 + i] = (int32_t)(F == TextFormat::Json ? c : textenc::csv_extra_of(c >> 1, c & 1u));
    }
    if (tid == 0 && s_any) atomicOr(any, 1u);
}

// ---- one value ---------------------------------------------------------------------------------------------------------------------------------------------
struct EncVal {
    uint64_t bits;     // a number's 64 bits (Int32 sign-extended)
    int32_t begin;     // Utf8: where the value's bytes begin
    uint32_t len;      // Utf8: their count
    uint32_t extra;    // Utf8: what escaping / quoting adds (textenc.hpp)
    bool valid;
};

// Loads value `row` of the column; returns its length as text.  *bad: a CSV timestamp outside the years 0000..9999 (length 0)
template <TextFormat F>
__device__ __forceinline__ uint64_t load_value(const EncCol &c, int64_t row, EncVal *v, bool *bad) {
    v->valid = !c.valid || c.valid[row] != 0;
    v->bits = 0;
    v->begin = 0;
    v->len = v->extra = 0;
    if (c.type == kTextUtf8) {
        const int32_t b = c.off[row], e = c.off[row + 1];
        v->begin = b;
        v->len = e > b ? (uint32_t)(e - b) : 0u;
        if (v->valid && v->len && *c.any) v->extra = (uint32_t)c.extra[row];
        return textenc::utf8_len(F, v->valid, v->len, v->extra);
    }
    if (c.type == kTextInt32) v->bits = (uint64_t)(int64_t) static_cast<const int32_t *>(c.values)[row];
    else v->bits = static_cast<const uint64_t *>(c.values)[row];
    if (F == TextFormat::Csv && c.type == kTextTimestampMs && v->valid && !numtext_ts_in_range((int64_t)v->bits)) {
        *bad = true;
        return 0;
    }
    return textenc::num_len(F, c.type, v->valid, v->bits);
}

// ---- length pass ---------------------------------------------------------------------------------------------------------------------------------------------
template <TextFormat F>
__global__ __launch_bounds__(kBlock) void textenc_len_kernel(const EncCol *__restrict__ cols, int32_t n_cols, int64_t rows, uint32_t pre_total,
                                                             uint32_t *__restrict__ row_len, uint32_t *__restrict__ counts, unsigned long long *err,
                                                             uint32_t *h_flag) {
    const int64_t row = (int64_t)blockIdx.x * kEncTile + threadIdx.x;
    uint64_t len = 0;
    if (row < rows) {
        uint64_t sum = 0;
        for (int32_t c = 0; c < n_cols; ++c) {
            EncVal v;
            bool bad = false;
            sum += load_value<F>(cols[c], row, &v, &bad);
            if (bad) {
                atomicMin(err, ((unsigned long long)row << 8) | (unsigned long long)c);
                __atomic_store_n(h_flag, 1u, __ATOMIC_RELAXED);   // (pinned host memory; every failing lane stores the same word)
            }
        }
        len = textenc::row_len(F, pre_total, sum);
        len = len < kLenCap ? len : kLenCap;
        row_len[row] = (uint32_t)len;
    }
    uint64_t incl = wave_incl_scan_u64(len);   // (64 rows of at most 2^31)
    incl = incl < kLenCap ? incl : kLenCap;
    if (lane_id() == 63) counts[(size_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)] = (uint32_t)incl;
}

// ---- emit pass -------------------------------------------------------------------------------------------------------------------------------------------------
// byte k of the words
__device__ __forceinline__ uint8_t pre_byte(const uint32_t *__restrict__ pre, uint32_t k) { return (uint8_t)(pre[k >> 2] >> (8u * (k & 3u))); }

// The pl bytes of `pre` (uniform: the words sit in scalar registers) at stage byte q: the words move up q & 3 bytes by funnel shift and land as ALIGNED
// dwords where all four bytes are theirs, byte by byte at the two ends
__device__ __forceinline__ void place_pre(uint8_t *stage, uint32_t q, const uint32_t *__restrict__ pre, uint32_t pl) {
    const uint32_t lo = q & 3u, hi = lo + pl;   // bytes [lo, hi) of the aligned dwords from q - lo on
    uint8_t *d = stage + (q - lo);
    const uint32_t nw = (pl + 3u) >> 2;
    uint32_t prev = 0;
    for (uint32_t j = 0; j <= nw; ++j) {
        const uint32_t cur = j < nw ? pre[j] : 0u;
        const uint32_t b0 = 4u * j;
        if (b0 < hi) {
            const uint32_t w = lo ? __funnelshift_r(prev, cur, 32u - 8u * lo) : cur;
            if (b0 >= lo && b0 + 4u <= hi) {
                *reinterpret_cast<uint32_t *>(d + b0) = w;
            } else {
                for (uint32_t t = 0; t < 4u; ++t)
                    if (b0 + t >= lo && b0 + t < hi) d[b0 + t] = (uint8_t)(w >> (8u * t));
            }
        }
        prev = cur;
    }
}

// what a source byte of a Utf8 value becomes: out[0 .. n)
template <TextFormat F>
__device__ __forceinline__ uint32_t expand(uint32_t b, uint8_t *out) {
    if (F == TextFormat::Json) return textenc::json_escape(b, out);
    out[0] = (uint8_t)b;
    out[1] = (uint8_t)'"';
    return b == 0x22u ? 2u : 1u;
}

// 0x80 in every byte of w that an escape / a doubling replaces
template <TextFormat F>
__device__ __forceinline__ uint32_t class_bytes(uint32_t w) {
    const uint32_t q = textenc::equal_bytes(w, 0x22u);
    return F == TextFormat::Json ? q | textenc::equal_bytes(w, 0x5Cu) | textenc::zero_bytes(w & 0xe0e0e0e0u) : q;
}

// A Utf8 value, all of it inside the stage, from stage byte q on; returns where it ends.  ONE loop for values with and without class bytes (lanes of
// either kind run it together).  The source is read byte by byte up to the first 4-byte boundary of its ADDRESS, then in dwords that lie wholly inside
// the value (so: inside the column's buffer); a dword without a class byte goes out whole when the stage position is aligned too.  `look` (uniform): the
// column holds a class byte somewhere; without one nothing is tested.
template <TextFormat F>
__device__ __forceinline__ uint32_t copy_value(uint8_t *stage, uint32_t q, const uint8_t *__restrict__ src, uint32_t len, bool look) {
    auto one = [&](uint32_t b) {
        const bool cls = look && (F == TextFormat::Json ? textenc::json_is_class(b) : b == 0x22u);
        if (!cls) {
            stage[q++] = (uint8_t)b;
        } else {
            uint8_t o[6];
            const uint32_t n = expand<F>(b, o);
            for (uint32_t j = 0; j < n; ++j) stage[q + j] = o[j];
            q += n;
        }
    };
    uint32_t k = 0;
    const uint32_t lead = (4u - (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3u)) & 3u;
    for (; k < len && k < lead; ++k) one(src[k]);
    for (; k + 4u <= len; k += 4u) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(src + k);
        if (!look || class_bytes<F>(w) == 0u) {
            if ((q & 3u) == 0u) {
                *reinterpret_cast<uint32_t *>(stage + q) = w;
            } else {
                stage[q] = (uint8_t)w;
                stage[q + 1] = (uint8_t)(w >> 8);
                stage[q + 2] = (uint8_t)(w >> 16);
                stage[q + 3] = (uint8_t)(w >> 24);
            }
            q += 4u;
        } else {
            one(w & 0xffu);
            one((w >> 8) & 0xffu);
            one((w >> 16) & 0xffu);
            one(w >> 24);
        }
    }
    for (; k < len; ++k) one(src[k]);
    return q;
}

// a number at stage byte q, all of it inside the stage
template <TextFormat F>
__device__ __forceinline__ void place_number(uint8_t *stage, uint32_t q, int32_t type, uint64_t bits) {
    if (type == kTextInt32) numtext_place<3, 3>(stage, q, numtext_i32((int32_t)(int64_t)bits));
    else if (type == kTextUInt64) numtext_place<5, 5>(stage, q, numtext_u64(bits, false));
    else if (type == kTextTimestampMs && F == TextFormat::Csv) numtext_place<6, 1>(stage, q, numtext_ts((int64_t)bits));
    else numtext_place<5, 5>(stage, q, numtext_i64((int64_t)bits));
}

template <int kWords, class Put>
__device__ __forceinline__ void put_text(const NumText<kWords> &t, uint32_t pos, Put put) {
    for (uint32_t i = 0; i < t.len; ++i) put(pos + i, numtext_byte(t, i));
}
// the same number byte by byte through the clipped store
template <TextFormat F, class Put>
__device__ __forceinline__ void put_number(int32_t type, uint64_t bits, uint32_t pos, Put put) {
    if (type == kTextInt32) put_text(numtext_i32((int32_t)(int64_t)bits), pos, put);
    else if (type == kTextUInt64) put_text(numtext_u64(bits, false), pos, put);
    else if (type == kTextTimestampMs && F == TextFormat::Csv) put_text(numtext_ts((int64_t)bits), pos, put);
    else put_text(numtext_i64((int64_t)bits), pos, put);
}

template <TextFormat F>
__global__ __launch_bounds__(kBlock) void textenc_emit_kernel(const EncCol *__restrict__ cols, int32_t n_cols, int64_t rows, const uint32_t *__restrict__ row_len,
                                                              const uint32_t *__restrict__ counts, const uint64_t *__restrict__ tile_base, uint64_t head,
                                                              uint8_t *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[kEncStage];
    const int wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * kEncTile + threadIdx.x;
    const uint32_t mine = row < rows ? row_len[row] : 0u;
    const uint4 wc = *reinterpret_cast<const uint4 *>(counts + (size_t)blockIdx.x * kWavesPerBlock);
    const uint32_t tile_bytes = wc.x + wc.y + wc.z + wc.w;   // (the call's total is below 2^31)
    const uint64_t base = head + tile_base[blockIdx.x];
    const uint32_t start = (wave > 0 ? wc.x : 0u) + (wave > 1 ? wc.y : 0u) + (wave > 2 ? wc.z : 0u) + wave_incl_scan_u32(mine) - mine;
    // positions are relative to the 16-byte boundary at or below the tile's first byte: the tile's bytes are [phase, end)
    const uint32_t phase = (uint32_t)(base & 15);
    const uint32_t end = phase + tile_bytes;
    uint8_t *gout = out + (base - phase);
    const uint32_t row_pos = phase + start;
    uint32_t pos = row_pos;          // where the cursor's next element begins
    int32_t c = 0, part = 0;         // the cursor: column; 0 = the bytes in front, 1 = the value's head, 2 = a string's bytes, 3 = its closing quote
    uint32_t i = 0;                  // part 2: the next source byte
    bool done = row >= rows;
    for (uint32_t R0 = 0; R0 < end; R0 += kEncStage) {   // (block-uniform)
        const uint32_t R1 = R0 + kEncStage;
        auto put = [&](uint32_t p, uint8_t b) {
            if (p >= R0 && p < R1) s_stage[p - R0] = b;
        };
        // One sweep over the columns, the SAME column in every lane (the table arrives as scalar loads, the type switch is uniform); a lane acts where
        // its cursor stands.  A cursor only moves forward, so a lane that stops on the round's seam sits out the rest of the sweep.
        for (int32_t cu = 0; cu < n_cols; ++cu) {
            const EncCol &col = cols[cu];
            if (done || c != cu || pos >= R1) continue;
            EncVal v;
            bool bad = false;
            const uint64_t vlen = load_value<F>(col, row, &v, &bad);
            const bool text = col.type == kTextUtf8 && v.valid;
            const bool quoted = text && (F == TextFormat::Json || textenc::csv_utf8_quoted(v.len, v.extra));
            const uint32_t pl = (uint32_t)col.pre_len;
            if (part == 0 && pos >= R0 && (uint64_t)pos + pl + vlen <= R1) {   // the whole column lies inside the round
                uint32_t q = pos - R0;
                place_pre(s_stage, q, col.pre, pl);
                q += pl;
                if (!v.valid) {
                    if (F == TextFormat::Json) {
                        s_stage[q] = (uint8_t)'n';
                        s_stage[q + 1] = (uint8_t)'u';
                        s_stage[q + 2] = (uint8_t)'l';
                        s_stage[q + 3] = (uint8_t)'l';
                    }
                } else if (!text) {
                    place_number<F>(s_stage, q, col.type, v.bits);
                } else {
                    if (quoted) s_stage[q++] = (uint8_t)'"';
                    q = copy_value<F>(s_stage, q, col.bytes + v.begin, v.len, *col.any != 0u);
                    if (quoted) s_stage[q] = (uint8_t)'"';
                }
                pos += pl + (uint32_t)vlen;
                ++c;
                continue;
            }
            // on a seam: element by element, every store clipped to the round; an element that crosses R1 stays the cursor's
            if (part == 0) {
                for (uint32_t k = 0; k < pl; ++k) put(pos + k, pre_byte(col.pre, k));
                if (pos + pl > R1) continue;
                pos += pl;
                part = 1;
            }
            if (part == 1) {
                if (!text) {
                    const uint32_t n = (uint32_t)vlen;   // at most 23
                    if (!v.valid) {
                        if (F == TextFormat::Json) {
                            put(pos, (uint8_t)'n');
                            put(pos + 1, (uint8_t)'u');
                            put(pos + 2, (uint8_t)'l');
                            put(pos + 3, (uint8_t)'l');
                        }
                    } else {
                        put_number<F>(col.type, v.bits, pos, put);
                    }
                    if (pos + n > R1) continue;
                    pos += n;
                    part = 0;
                    ++c;
                    continue;
                }
                if (quoted) {
                    put(pos, (uint8_t)'"');
                    if (pos + 1 > R1) continue;
                    pos += 1;
                }
                part = 2;
                i = 0;
            }
            if (part == 2) {
                const uint8_t *__restrict__ src = col.bytes + v.begin;
                bool stop = false;
                while (i < v.len) {
                    uint8_t o[6];
                    const uint32_t n = expand<F>(src[i], o);
                    for (uint32_t j = 0; j < n; ++j) put(pos + j, o[j]);
                    if (pos + n > R1) {
                        stop = true;
                        break;
                    }
                    pos += n;
                    ++i;
                }
                if (stop) continue;
                part = 3;
            }
            if (quoted) {   // part 3
                put(pos, (uint8_t)'"');
                if (pos + 1 > R1) continue;
                pos += 1;
            }
            part = 0;
            ++c;
        }
        if (!done && c == n_cols && pos < R1) {   // the row's end
            uint32_t n;
            if (F == TextFormat::Json) {
                put(pos, (uint8_t)'}');
                put(pos + 1, (uint8_t)'\n');
                n = 2;
            } else if (pos == row_pos) {   // a record that would be empty
                put(pos, (uint8_t)'"');
                put(pos + 1, (uint8_t)'"');
                put(pos + 2, (uint8_t)'\n');
                n = 3;
            } else {
                put(pos, (uint8_t)'\n');
                n = 1;
            }
            if (pos + n <= R1) {
                pos += n;
                done = true;
            }
        }
        __syncthreads();
        const uint32_t lim = end - R0 < (uint32_t)kEncStage ? end - R0 : (uint32_t)kEncStage;
        for (uint32_t o = threadIdx.x * 16; o < lim; o += kBlock * 16) {
            const uint32_t g = R0 + o;
            if (g >= phase && g + 16 <= end) {
                stream_store4(gout + g, *reinterpret_cast<const uint4 *>(s_stage + o));
            } else {   // the tile's first / last chunk is shared with the neighbouring tile: only this tile's bytes
                for (uint32_t b = (g < phase ? phase : g); b < g + 16 && b < end; ++b) gout[b] = s_stage[b - R0];
            }
        }
        __syncthreads();
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------------
const char *type_name(int32_t t) {
    static const char *names[] = {"Int32", "Int64", "UInt64", "Float64", "Timestamp(ms)", "Utf8"};
    return t >= 0 && t <= kTextUtf8 ? names[t] : "unknown";
}

std::string json_string(const char *s) {
    std::string o = "\"";
    for (const char *p = s; *p; ++p) {
        uint8_t e[6];
        const uint32_t n = textenc::json_escape((uint8_t)*p, e);
        o.append(reinterpret_cast<const char *>(e), n);
    }
    return o + "\"";
}

std::string csv_string(const char *s, uint32_t delim) {
    bool quote = *s == 0;
    for (const char *p = s; *p; ++p) quote = quote || textenc::csv_is_special((uint8_t)*p, delim);
    if (!quote) return s;
    std::string o = "\"";
    for (const char *p = s; *p; ++p) {
        o.push_back(*p);
        if (*p == '"') o.push_back('"');
    }
    return o + "\"";
}

template <TextFormat F>
int encode(flockgpu_ctx *ctx, const flockgpu_text_column *cols, int32_t n_cols, int64_t rows, uint32_t delim, bool has_header, flockgpu_text_result *out) {
    const char *who = F == TextFormat::Json ? "json encode" : "csv encode";
    if (!ctx) return FLOCKGPU_ERR_INVALID;
    if (!out) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: null argument", who);
    *out = flockgpu_text_result{};
    if (!cols || n_cols < 1) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: no columns", who);
    if (n_cols > kTextEncMaxCols)
        return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: column %d ('%s'): more than %d columns", who, kTextEncMaxCols,
                    cols[kTextEncMaxCols].name ? cols[kTextEncMaxCols].name : "", kTextEncMaxCols);
    if (F == TextFormat::Csv && (delim >= 0x80u || delim == (uint32_t)'"' || delim == (uint32_t)'\r' || delim == (uint32_t)'\n'))
        return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: the delimiter is an ASCII byte other than '\"', CR and LF (got 0x%02x)", who, delim);
    if (rows < 0 || rows >= (int64_t(1) << 31)) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: %lld rows: not in [0, 2^31)", who, (long long)rows);
    for (int c = 0; c < n_cols; ++c) {
        const flockgpu_text_column &col = cols[c];
        const size_t nl = col.name ? strlen(col.name) : 0;
        if (nl == 0 || nl > (size_t)kTextEncMaxName)
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: column %d: a name is 1 to %d bytes (got %zu)", who, c, kTextEncMaxName, nl);
        if (col.type == kTextFloat64)
            return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: column %d ('%s'): Float64 has no shortest round-trip text form on the device", who, c, col.name);
        if (col.type < kTextInt32 || col.type > kTextUtf8) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: column %d ('%s'): unknown type %d", who, c, col.name, col.type);
        if (col.type == kTextUtf8 && !col.utf8.offsets) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: column %d ('%s'): a Utf8 column without offsets", who, c, col.name);
        if (col.type != kTextUtf8 && rows > 0 && !col.values) return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: column %d ('%s'): a %s column without values", who, c, col.name, type_name(col.type));
    }
    FG_HIP(ctx, hipSetDevice(ctx->device));

    // ---- the column table, the header record
    EncCol *d_cols = nullptr, *h_cols = nullptr;
    uint32_t *d_any = nullptr;
    FG_TRY(arena_get_t(ctx, "textenc.cols", kTextEncMaxCols, &d_cols));
    FG_TRY(pinned_get_t(ctx, "textenc.cols", kTextEncMaxCols, &h_cols));
    FG_TRY(arena_get_t(ctx, "textenc.any", kTextEncMaxCols, &d_any));
    std::string header;
    uint32_t pre_total = 0;
    int n_utf8 = 0;
    for (int c = 0; c < n_cols; ++c) {
        const flockgpu_text_column &col = cols[c];
        EncCol &e = h_cols[c];   // (the stream is idle: every call ends its uploads with a wait)
        e = EncCol{};
        e.type = col.type;
        e.valid = col.valid;
        e.any = d_any + c;
        std::string pre;
        if (F == TextFormat::Json) pre = (c == 0 ? "{" : ",") + json_string(col.name) + ":";
        else if (c > 0) pre.assign(1, (char)delim);
        e.pre_len = (int32_t)pre.size();   // at most 2 + 6 * 31 + 2
        std::memcpy(e.pre, pre.data(), pre.size());
        pre_total += (uint32_t)pre.size();
        if (col.type == kTextUtf8) {
            char name[48];
            int32_t *extra = nullptr;
            snprintf(name, sizeof name, "textenc.extra.%d", c);
            FG_TRY(arena_get_t(ctx, name, (size_t)rows + 4, &extra));
            e.off = col.utf8.offsets;
            e.bytes = col.utf8.data;
            e.extra = extra;
            ++n_utf8;
        } else {
            e.values = col.values;
        }
        if (F == TextFormat::Csv && has_header) header += (c ? std::string(1, (char)delim) : std::string()) + csv_string(col.name, delim);
    }
    if (F == TextFormat::Csv && has_header) header += "\n";
    const uint64_t head = header.size();
    uint8_t *d_head = nullptr, *h_head = nullptr;
    FG_TRY(arena_get_t(ctx, "textenc.head", (size_t)head + 16, &d_head));
    FG_TRY(pinned_get_t(ctx, "textenc.head", (size_t)head + 16, &h_head));
    if (head) {
        std::memcpy(h_head, header.data(), head);
        FG_HIP(ctx, hipMemcpyAsync(d_head, h_head, head, hipMemcpyHostToDevice, ctx->stream));
    }

    // ---- class and length passes, the scan
    const int64_t tiles = div_up(rows, kEncTile);
    uint32_t *row_len = nullptr, *counts = nullptr, *h_flag = nullptr;
    uint64_t *tile_base = nullptr, *h_total = nullptr;
    unsigned long long *d_err = nullptr;
    FG_TRY(arena_get_t(ctx, "textenc.row_len", (size_t)rows + 4, &row_len));
    FG_TRY(arena_get_t(ctx, "textenc.counts", (size_t)std::max<int64_t>(tiles, 1) * kWavesPerBlock, &counts));
    FG_TRY(arena_get_t(ctx, "textenc.base", (size_t)tiles + 1, &tile_base));
    FG_TRY(arena_get_t(ctx, "textenc.err", 2, &d_err));
    FG_TRY(pinned_get_t(ctx, "textenc.total", 2, &h_total));
    FG_TRY(pinned_get_t(ctx, "textenc.flag", 4, &h_flag));
    *h_total = 0;
    __atomic_store_n(h_flag, 0u, __ATOMIC_RELAXED);   // (no kernel that writes it is in flight: the call that queued one has waited behind it)
    uint64_t total = 0;
    if (rows > 0) {
        FG_HIP(ctx, hipMemcpyAsync(d_cols, h_cols, sizeof(EncCol) * (size_t)n_cols, hipMemcpyHostToDevice, ctx->stream));
        FG_TRY(fill_words(ctx, FillList().add(d_any, 0u, kTextEncMaxCols).add(d_err, 0xFFFFFFFFu, 2)));
        if (n_utf8) {
            LaunchScope ls(ctx, "textenc_class_kernel");
            for (int c = 0; c < n_cols; ++c) {
                if (cols[c].type != kTextUtf8) continue;
                hipLaunchKernelGGL(textenc_class_kernel<F>, dim3((unsigned)div_up(rows, kClsRows)), dim3(kBlock), 0, ctx->stream, cols[c].utf8.offsets,
                                   cols[c].utf8.data, rows, delim, const_cast<int32_t *>(h_cols[c].extra), d_any + c);
            }
        }
        FG_TRY(check_launch(ctx, "textenc_class_kernel"));
        {
            LaunchScope ls(ctx, "textenc_len_kernel");
            hipLaunchKernelGGL(textenc_len_kernel<F>, dim3((unsigned)tiles), dim3(kBlock), 0, ctx->stream, d_cols, n_cols, rows, pre_total, row_len, counts, d_err, h_flag);
        }
        FG_TRY(check_launch(ctx, "textenc_len_kernel"));
        FG_TRY(launch_tile_scan(ctx, counts, (int32_t)tiles, tile_base, nullptr, 0, nullptr));
        FG_TRY(publish_words(ctx, PublishList().add(h_total, tile_base + tiles, 2)));
        FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (__atomic_load_n(h_flag, __ATOMIC_RELAXED)) {   // (CSV only) the failure path alone pays for a copy of the device word
            unsigned long long first = 0;
            FG_HIP(ctx, hipMemcpy(&first, d_err, sizeof first, hipMemcpyDeviceToHost));
            const int col = (int)(first & 0xFF);
            return fail(ctx, FLOCKGPU_ERR_INVALID, "%s: record %lld: column %d ('%s'): a Timestamp(ms) outside the years 0000 to 9999 has no text form", who,
                        (long long)(first >> 8) + 1 + (has_header ? 1 : 0), col, col < n_cols ? cols[col].name : "");
        }
        total = *h_total;
    } else if (head) {
        FG_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (h_head is the next call's to write)
    }
    const uint64_t n_bytes = head + total;
    if (n_bytes >= (uint64_t(1) << 31) - 16)
        return fail(ctx, FLOCKGPU_ERR_UNSUPPORTED, "%s: the text comes to %llu bytes; a call writes fewer than 2^31 - 16 (Arrow Utf8 offsets and the decoders are int32)", who,
                    (unsigned long long)n_bytes);

    // ---- emit
    uint8_t *text = nullptr;
    const size_t padded = ((size_t)n_bytes + 15) & ~size_t(15);
    FG_TRY(arena_get_t(ctx, "textenc.text", padded + 16, &text));
    if (padded > n_bytes) FG_HIP(ctx, hipMemsetAsync(text + n_bytes, 0, padded - n_bytes, ctx->stream));
    if (head) FG_HIP(ctx, hipMemcpyAsync(text, d_head, head, hipMemcpyDeviceToDevice, ctx->stream));
    if (rows > 0) {
        {
            LaunchScope ls(ctx, "textenc_emit_kernel");
            hipLaunchKernelGGL(textenc_emit_kernel<F>, dim3((unsigned)tiles), dim3(kBlock), 0, ctx->stream, d_cols, n_cols, rows, row_len, counts, tile_base, head, text);
        }
        FG_TRY(check_launch(ctx, "textenc_emit_kernel"));
    }
    out->text = text;
    out->n_bytes = (int64_t)n_bytes;
    return FLOCKGPU_OK;
}

}  // namespace

extern "C" {

int flockgpu_json_lines_encode(flockgpu_ctx *ctx, const flockgpu_text_column *cols, int32_t n_cols, int64_t rows, flockgpu_text_result *out) {
    return encode<TextFormat::Json>(ctx, cols, n_cols, rows, 0u, false, out);
}

int flockgpu_csv_encode(flockgpu_ctx *ctx, const flockgpu_text_column *cols, int32_t n_cols, int64_t rows, const flockgpu_csv_options *opt,
                        flockgpu_text_result *out) {
    if (ctx && !opt) return fail(ctx, FLOCKGPU_ERR_INVALID, "csv encode: null argument");
    return encode<TextFormat::Csv>(ctx, cols, n_cols, rows, opt ? opt->delimiter : (uint32_t)',', opt && opt->has_header, out);
}

}  // extern "C"
