// Bit arithmetic of the text slice functions (textslice.hpp): the class masks of a 16-byte chunk and the position of the k-th set bit of a mask word.
// Plain C++ that compiles on the host and on the device; tests/cpp/textslice_bits_test.cpp checks every function against a byte-by-byte / bit-by-bit
// loop.  A chunk's mask has bit k set where byte k of the chunk belongs to the class:
//   lead    the byte is not 10xxxxxx: it begins a code point (A-L2)              -- left / right
//   equal   the byte is the (one-byte) delimiter                                   -- split_part
//   outside the byte is not one of a set of ASCII characters (a 128-bit table; every byte >= 0x80 is outside)  -- ltrim / rtrim / btrim
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FG_SLICE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define FG_SLICE_HD inline
#endif

namespace flockgpu {
namespace slicebits {

// bit 7 of every byte of w -> bits 0..3
FG_SLICE_HD uint32_t gather_bit7(uint32_t m) { return ((m >> 7) & 1u) | ((m >> 14) & 2u) | ((m >> 21) & 4u) | ((m >> 28) & 8u); }

// bit k: byte k of w is not a continuation byte
FG_SLICE_HD uint32_t lead_mask4(uint32_t w) {
    const uint32_t cont = w & (~w << 1) & 0x80808080u;   // bit 7 of a byte: 1 where the byte is 10xxxxxx
    return gather_bit7(~cont & 0x80808080u);
}

// bit k: byte k of w equals c.  (x = w ^ cccc has a zero byte there; the carry-free zero-byte test: the low seven bits are added to 0x7f inside
// their own byte, so no carry crosses into the neighbour)
FG_SLICE_HD uint32_t equal_mask4(uint32_t w, uint8_t c) {
    const uint32_t x = w ^ (0x01010101u * c);
    const uint32_t nonzero = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
    return gather_bit7(~nonzero & 0x80808080u);
}

// A set of ASCII characters: bit c of the 128-bit table
struct AsciiSet {
    uint64_t lo, hi;   // characters 0..63, 64..127
};
FG_SLICE_HD void ascii_set_add(AsciiSet &s, uint32_t byte) { (byte & 64u ? s.hi : s.lo) |= uint64_t(1) << (byte & 63u); }
FG_SLICE_HD bool ascii_set_has(const AsciiSet &s, uint32_t byte) { return byte < 128u && (((byte & 64u ? s.hi : s.lo) >> (byte & 63u)) & 1u) != 0; }

// bit k: byte k of w is not in the set
FG_SLICE_HD uint32_t outside_mask4(uint32_t w, const AsciiSet &s) {
    uint32_t m = 0;
    for (int k = 0; k < 4; ++k) m |= (uint32_t)!ascii_set_has(s, (w >> (8 * k)) & 0xffu) << k;
    return m;
}

enum ByteClass : int { kLead = 0, kEqual = 1, kOutside = 2 };

// the 16-bit mask of a chunk held as four little-endian dwords
template <int kClass>
FG_SLICE_HD uint32_t chunk_mask(uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint8_t delim, const AsciiSet &set) {
    if (kClass == kLead) return lead_mask4(x) | (lead_mask4(y) << 4) | (lead_mask4(z) << 8) | (lead_mask4(w) << 12);
    if (kClass == kEqual) return equal_mask4(x, delim) | (equal_mask4(y, delim) << 4) | (equal_mask4(z, delim) << 8) | (equal_mask4(w, delim) << 12);
    return outside_mask4(x, set) | (outside_mask4(y, set) << 4) | (outside_mask4(z, set) << 8) | (outside_mask4(w, set) << 12);
}

FG_SLICE_HD int popcount64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}

// Position of the k-th set bit of x, k = 0 for the lowest; k < popcount64(x) is the caller's to ensure (else 64).  A binary descent over the halves:
// six popcounts, no loop over the bits.
FG_SLICE_HD int select64(uint64_t x, int k) {
    if (k < 0 || k >= popcount64(x)) return 64;
    int pos = 0;
    for (int width = 32; width >= 1; width >>= 1) {
        const uint64_t low = x & ((uint64_t(1) << width) - 1);
        const int c = popcount64(low);
        if (k >= c) {
            k -= c;
            x >>= width;
            pos += width;
        } else {
            x = low;
        }
    }
    return pos;
}

// Position of the highest set bit of x != 0
FG_SLICE_HD int highest64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return 63 - __clzll((long long)x);
#else
    return 63 - __builtin_clzll(x);
#endif
}

// x restricted to the positions [a, b) of the 64 the word covers from position `lo` on (a < b, [a, b) meets [lo, lo + 64))
FG_SLICE_HD uint64_t clip_word(uint64_t x, int64_t lo, int64_t a, int64_t b) {
    if (a > lo) x &= ~uint64_t(0) << (a - lo);
    if (b < lo + 64) x &= ~uint64_t(0) >> (lo + 64 - b);
    return x;
}

}  // namespace slicebits
}  // namespace flockgpu
