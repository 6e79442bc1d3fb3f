// Float64 MIN / MAX through unsigned 64-bit keys of the same order, shared by the GROUP BY tables (relops.hip) and the wide GROUP BY pass
// (groupwide.hip): negative values have all their bits flipped, the others their sign bit set.  No NaN among the inputs (relops.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace flockgpu {

__device__ __forceinline__ uint64_t f64_order_key(double d) {
    const uint64_t b = (uint64_t)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ uint64_t f64_from_order_key(uint64_t k) { return (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k; }

}  // namespace flockgpu
