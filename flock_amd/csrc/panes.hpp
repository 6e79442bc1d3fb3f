// Event-time panes (panes.hip): a batch of rows cut into the panes of a hopping window by a timestamp column, on the device
// (flockgpu_pane_split, include/flockgpu.h).  The host-side twin is WindowSchedule / window_epochs, which cut panes from the generator's epoch
// structure; decoded text has no such structure, only a timestamp column.
//
// What the operator assumes and guarantees:
//   A-PN1  pane(t) = floor((t - origin) / hop), rounding towards minus infinity: t = origin - 1 lies in pane -1.
//   A-PN2  t - origin is formed exactly (65 bits: a sign and a 64-bit magnitude), for every Int64 t and origin.
//   A-PN3  a pane id that does not fit Int64 is refused (FLOCKGPU_ERR_INVALID); pane() is monotone in t, so only the panes of min t and max t
//          have to be looked at.
//   A-PN4  hop > 0; 1 <= capacity <= kPaneMaxCapacity; 0 <= rows < 2^31.
//   A-PN5  first_pane = pane(min t); n_panes = pane(max t) - first_pane + 1; more than `capacity` panes are refused (FLOCKGPU_ERR_UNSUPPORTED):
//          one garbage timestamp would otherwise ask for billions of panes.  Nothing is written to `bounds` by a refused call.
//   A-PN6  a validity byte of 0 anywhere refuses the call (FLOCKGPU_ERR_INVALID) and names the FIRST such row: a row without a time has no pane.
//   A-PN7  rows are "in pane order" when pane ids never decrease along the rows; timestamps inside a pane may come in any order.  Row i can break
//          the order only where t[i] < t[i - 1] (pane() is monotone), so only such a descent has its two pane ids compared: the streaming pass
//          divides nowhere else.
//   A-PN8  in pane order, pane first_pane + k is rows [bounds[k], bounds[k + 1]) of the input itself and no row list is made; bounds[k] is the
//          lower bound of threshold(first_pane + k) = origin + (first_pane + k) * hop in the timestamp column: t[i] >= threshold is monotone in i
//          exactly when the rows are in pane order.  Every threshold that is searched lies in (min t, max t], so it fits Int64.
//   A-PN9  otherwise the row list is a STABLE permutation: pane first_pane + k is the input rows row_list[bounds[k] .. bounds[k + 1]), ascending
//          inside the pane.  The list is the context's and valid until the next call on it.
//   A-PN10 bounds[0] = 0, bounds[n_panes] = rows; an empty pane in between has bounds[k] == bounds[k + 1]; rows == 0: n_panes = 0, first_pane = 0,
//          nothing is launched.
//   A-PN11 time_ms needs 8-byte alignment only, validity bytes none; nothing outside [time_ms, time_ms + rows) and [valid, valid + rows) is read.
//
// The arithmetic below is plain C++ for host and device (tests/cpp/panes_test.cpp checks it on the host).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FG_PANE_HD __host__ __device__ inline
#else
#define FG_PANE_HD inline
#endif

struct flockgpu_ctx;

namespace flockgpu {
namespace panes {

constexpr int kPaneTile = 8192;            // T: rows of the timestamp column per workgroup tile of the streaming pass
constexpr int kPaneMaxCapacity = 65536;    // panes per call, at most

// A 65-bit signed integer: -mag when neg (mag != 0 then), else mag.
struct Wide {
    uint64_t mag;
    bool neg;
};

// a - b, exactly (A-PN2).
FG_PANE_HD Wide exact_diff(int64_t a, int64_t b) {
    const uint64_t ua = (uint64_t)a, ub = (uint64_t)b;
    return a >= b ? Wide{ua - ub, false} : Wide{ub - ua, true};
}
// floor(d / hop) for hop > 0 (A-PN1): the quotient of a 65-bit value is a 65-bit value.
FG_PANE_HD Wide floor_div(Wide d, int64_t hop) {
    const uint64_t h = (uint64_t)hop;
    if (!d.neg) return Wide{d.mag / h, false};
    const uint64_t q = d.mag / h;
    return Wide{q + (d.mag - q * h != 0 ? 1u : 0u), true};   // -ceil(mag / hop); mag >= 1, so the result is not -0
}
FG_PANE_HD Wide pane_wide(int64_t t, int64_t origin, int64_t hop) { return floor_div(exact_diff(t, origin), hop); }
FG_PANE_HD bool wide_less(Wide a, Wide b) {
    if (a.neg != b.neg) return a.neg;
    return a.neg ? a.mag > b.mag : a.mag < b.mag;
}
// The Int64 fit (A-PN3): false when the value lies outside [-2^63, 2^63).
FG_PANE_HD bool wide_fits(Wide v, int64_t *out) {
    const uint64_t top = uint64_t(1) << 63;
    if (v.neg ? v.mag > top : v.mag >= top) return false;
    *out = (int64_t)(v.neg ? uint64_t(0) - v.mag : v.mag);
    return true;
}
// pane(t) as an Int64; false when it does not fit.
FG_PANE_HD bool pane_of(int64_t t, int64_t origin, int64_t hop, int64_t *pane) { return wide_fits(pane_wide(t, origin, hop), pane); }

// a * b of two unsigned 64-bit values as (hi, lo), from 32-bit halves.
FG_PANE_HD void mul_u64(uint64_t a, uint64_t b, uint64_t *hi, uint64_t *lo) {
    const uint64_t a0 = a & 0xffffffffu, a1 = a >> 32, b0 = b & 0xffffffffu, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffu) + (p10 & 0xffffffffu);
    *lo = (p00 & 0xffffffffu) | (mid << 32);
    *hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}
// threshold(p) = origin + p * hop, the smallest t of pane p, formed without overflow (A-PN8): false when it does not fit Int64 (p * hop alone
// may not fit where the sum does, so the product is kept as a sign and a 128-bit magnitude).
FG_PANE_HD bool pane_threshold(int64_t p, int64_t origin, int64_t hop, int64_t *out) {
    const bool neg = p < 0;
    uint64_t hi, lo;
    mul_u64(neg ? uint64_t(0) - (uint64_t)p : (uint64_t)p, (uint64_t)hop, &hi, &lo);
    if (hi) return false;   // |p * hop| >= 2^64: no Int64 origin brings the sum back
    // origin + (neg ? -lo : lo) as a 65-bit value
    const bool oneg = origin < 0;
    const uint64_t omag = oneg ? uint64_t(0) - (uint64_t)origin : (uint64_t)origin;
    Wide s;
    if (oneg == neg) {   // magnitudes add: the sum may pass 2^64
        const uint64_t m = omag + lo;
        if (m < omag) return false;
        s = Wide{m, m != 0 && neg};
    } else if (omag >= lo) {
        s = Wide{omag - lo, oneg && omag != lo};
    } else {
        s = Wide{lo - omag, neg};
    }
    return wide_fits(s, out);
}

}  // namespace panes

struct PaneSplit {
    int64_t first_pane = 0;
    int32_t n_panes = 0;
    const int32_t *row_list = nullptr;   // device, ctx-owned; nullptr: the rows are in pane order
};
// flockgpu_pane_split behind its argument checks (panes.hip); `bounds` has room for capacity + 1 entries and is written only on success.
int pane_split(flockgpu_ctx *ctx, const int64_t *time_ms, const uint8_t *valid, int64_t rows, int64_t origin_ms, int64_t hop_ms, int32_t capacity,
               int64_t *bounds, PaneSplit *out);

}  // namespace flockgpu
