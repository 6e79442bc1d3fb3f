// The chunk-wise emit of LONG Utf8 values, shared by the take (gather.hip utf8_emit_long_kernel) and the text-valued expressions (textsel.hip
// textsel_emit_long_kernel): a tile's values lie one after the other in ONE contiguous window of the output; LDS holds every value's END position in
// the window (s_end, by value index = output order) and a map from every 16-byte chunk of the window to the value that holds its first byte, written
// by the values themselves; every lane then makes whole 16-byte chunks of the OUTPUT from the one or two ALIGNED 16-byte source chunks that hold each
// piece, realigned in registers, and stores them aligned.  Where a value lies is the caller's: addr_of(v) = the address of value v's first byte.
// History and measurements: gather.hip, above utf8_emit_long_kernel.
#pragma once
#include "scan.hpp"

namespace flockgpu {

constexpr int kLongMapChunks = 8192;   // 16 KB of LDS: the chunk -> value map of a 128 KB output window

// The calling lane owns kMine values: value index[k] starts at window byte start[k] (= phase + its offset in the tile) and is len[k] bytes long.
// s_end[v] must hold every value's end before the call (the function's first barrier publishes it); window byte i is output byte gout + i, gout
// 16-byte aligned, the tile's bytes are [phase, end).  kTileValues: values of a tile (entries of s_end).
template <int kTileValues, int kMine, typename AddrOf>
__device__ __forceinline__ void utf8_emit_chunks(const uint32_t *s_end, AddrOf addr_of, uint16_t *s_first, const uint32_t (&start)[kMine], const uint32_t (&len)[kMine],
                                                 const uint32_t (&index)[kMine], uint32_t phase, uint32_t end, uint8_t *gout) {
    // bytes 0 .. x - 1 of a dword, x clamped to 0 .. 4 (no branches: a clamp, a 64-bit shift whose low word runs empty at x = 4, a complement)
    auto low_mask = [](int32_t x) -> uint32_t {
        const uint32_t c = (uint32_t)min(max(x, 0), 4);
        return ~(uint32_t)(0xffffffffull << (8u * c));
    };
    // sixteen chunk bytes from address A on (the byte at A lands on chunk byte 0; only chunk bytes a .. bnd - 1 are the value's -- the rest comes
    // back as whatever the two aligned chunks around them hold, or zero).  An aligned 16-byte chunk that holds at least one byte of the value
    // never crosses a page: only such chunks are read.
    auto realigned = [&](uintptr_t A, uint32_t a, uint32_t bnd, uint32_t (&V4)[4]) {
        const uint32_t sh = (uint32_t)(A & 15), qd = sh >> 2, bs = (sh & 3) * 8;
        const uint4 *q = reinterpret_cast<const uint4 *>(A & ~uintptr_t(15));
        uint4 c0 = make_uint4(0, 0, 0, 0), c1 = make_uint4(0, 0, 0, 0);
        if (bnd > a && sh + a < 16u) c0 = q[0];
        if (bnd > a && sh + bnd > 16u) c1 = q[1];
        // the window of five dwords that starts `qd` dwords into the eight: two rounds of bit-selects (by one dword, by two) -- a lane's qd is
        // its own, and the four-way choice written with ?: came back from the compiler as four divergent copies of everything behind it
        const uint32_t W[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        const uint32_t by1 = 0u - (qd & 1u), by2 = 0u - (qd >> 1);
        uint32_t X[7], V[5];
#pragma unroll
        for (int j = 0; j < 7; ++j) X[j] = (W[j + 1] & by1) | (W[j] & ~by1);
#pragma unroll
        for (int j = 0; j < 5; ++j) V[j] = (X[j + 2] & by2) | (X[j] & ~by2);
#pragma unroll
        for (int i = 0; i < 4; ++i) V4[i] = __funnelshift_r(V[i], V[i + 1], bs);
    };
    const uint32_t n_chunks = (end + 15u) >> 4;
    for (uint32_t cbase = 0; cbase < n_chunks; cbase += (uint32_t)kLongMapChunks) {   // (one round for tiles up to 128 KB: 128 bytes a value)
        const uint32_t cend = cbase + (uint32_t)kLongMapChunks < n_chunks ? cbase + (uint32_t)kLongMapChunks : n_chunks;
        // ---- every value names itself in the chunks whose first in-tile byte it holds: from the first 16-byte boundary at or behind its start
        // (the tile's very first chunk for the value that starts the tile) to the chunk of its last byte
        __syncthreads();   // (the lists above are complete; the previous round's map has been read)
#pragma unroll
        for (int k = 0; k < kMine; ++k) {
            if (len[k] == 0) continue;
            const uint32_t p0 = start[k], p1 = p0 + len[k];
            uint32_t c = p0 == phase ? 0u : (p0 + 15u) >> 4;
            const uint32_t c_last = (p1 - 1u) >> 4;
            if (c < cbase) c = cbase;
            for (; c <= c_last && c < cend; ++c) s_first[c - cbase] = (uint16_t)index[k];
        }
        __syncthreads();
        // ---- every lane makes whole chunks of the output
        for (uint32_t ci = cbase + threadIdx.x; ci < cend; ci += kBlock) {
            const uint32_t o = ci << 4, c_lo = o < phase ? phase : o, chi = o + 16 < end ? o + 16 : end;
            uint32_t v = s_first[ci - cbase];
            // the value the chunk starts in, and the one behind it: two pieces with ONE split between them is what a chunk of long values holds
            const uint32_t p0 = v ? s_end[v - 1] : phase, p1 = s_end[v], hi1 = p1 < chi ? p1 : chi;
            const uint32_t w = v + 1 < (uint32_t)kTileValues ? v + 1 : v;
            const uint32_t q1 = s_end[w], hi2 = hi1 < chi ? (q1 < chi ? q1 : chi) : hi1;
            uint32_t P1[4], P2[4], acc[4];
            realigned(addr_of(v) + o - p0, c_lo - o, hi1 - o, P1);
            realigned(addr_of(w) + o - p1, hi1 - o, hi2 - o, P2);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t m = low_mask((int32_t)(hi1 - o) - 4 * i);   // chunk bytes below the split are the first value's
                acc[i] = (P1[i] & m) | (P2[i] & ~m);
            }
            uint32_t pos = hi2;
            if (pos < chi) {   // (short values in a long column: a third piece and more, one by one under range masks)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] &= low_mask((int32_t)(pos - o) - 4 * i);
                for (v = w + 1; pos < chi; ++v) {
                    const uint32_t e = s_end[v], hi = e < chi ? e : chi;
                    if (hi <= pos) continue;   // (an empty value)
                    uint32_t P[4];
                    realigned(addr_of(v) + o - s_end[v - 1], pos - o, hi - o, P);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] |= P[i] & low_mask((int32_t)(hi - o) - 4 * i) & ~low_mask((int32_t)(pos - o) - 4 * i);
                    pos = hi;
                }
            }
            if (o >= phase && o + 16 <= end) {
                stream_store4(gout + o, make_uint4(acc[0], acc[1], acc[2], acc[3]));
            } else {  // the tile's first / last chunk is shared with the neighbouring tile: only this tile's bytes
                for (uint32_t c = c_lo; c < chi; ++c) gout[c] = (uint8_t)(acc[(c - o) >> 2] >> (8 * ((c - o) & 3)));
            }
        }
    }
}

}  // namespace flockgpu
