// Float64 MIN / MAX through unsigned 64-bit keys of the same order, shared by the GROUP BY tables (relops.hip) and the wide GROUP BY pass
// (groupwide.hip): negative values have all their bits flipped, the others their sign bit set.  No NaN among the inputs (relops.hpp).
// -0.0 lies below +0.0 in this order (A-FO4, relops.hpp).
//
// ORDER BY and the window's partition / peer tests take a Float64 key through f64_canonical_bits first (A-FO1, A-FO2): the two zeros are one
// value and every NaN is one value above +inf.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace flockgpu {

__device__ __forceinline__ uint64_t f64_order_key(double d) {
    const uint64_t b = (uint64_t)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ uint64_t f64_from_order_key(uint64_t k) { return (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k; }

// The bit pattern that stands for every double A-FO1 ties with `b`: -0.0 becomes +0.0, every NaN (either sign, any payload, quiet or
// signalling) becomes the positive quiet NaN 0x7FF8000000000000, whose order key lies above +inf's.  Everything else is itself.  Pure integer
// work: no floating-point mode (denormal flushing, NaN quieting) can touch it.
__device__ __forceinline__ uint64_t f64_canonical_bits(uint64_t b) {
    const uint64_t mag = b & 0x7fffffffffffffffull;
    if (mag > 0x7ff0000000000000ull) return 0x7ff8000000000000ull;
    return mag == 0 ? 0 : b;
}

}  // namespace flockgpu
