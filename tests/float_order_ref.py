"""How Float64 values order and compare: the A-FO rules of flock_amd/csrc/relops.hpp in plain Python, for tests/plan_interp.py and the tests of
tests/test_plan_float_edges.py.  A double is a Python float; its identity is its 64 bits (bits / from_bits), never `==`.

key(x)        A-FO1, ORDER BY: the comparison key of a non-NULL double.  Both zeros have one key, every NaN -- either sign, any payload, quiet or
              signalling -- has one key above +inf's.  Ascending order is sorted(..., key=key), which is stable; descending is the reverse on
              keys with ties still in input order (sorted(..., key=key, reverse=True) is that).
same(x, y)    A-FO2, the window's partitions and peer groups and ROW_NUMBER's runs: exactly when A-FO1 ties the two.
total_key(x)  A-FO4, MIN / MAX: the order of the kernels' unsigned order keys (orderkey.hpp f64_order_key): -0.0 below +0.0.  NaN among the inputs
              is outside the claim; the key is still total (a NaN with the sign bit set below -inf, one without above +inf).
SPECIALS      the pool of bit patterns the tests draw from."""
import struct

_SIGN = 1 << 63
_MASK = (1 << 64) - 1
_INF = 0x7FF0000000000000


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def is_nan_bits(b):
    return (b & ~_SIGN & _MASK) > _INF


def key(x):
    b = bits(x)
    if is_nan_bits(b):
        return (1, 0.0)
    return (0, 0.0 if (b & ~_SIGN & _MASK) == 0 else x)


def same(x, y):
    return key(x) == key(y)


def total_key(x):
    b = bits(x)
    return (~b & _MASK) if b & _SIGN else (b | _SIGN)


# NaNs: the positive quiet one, the one x86 gives for inf - inf, a signalling one, all ones
NANS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF]
SPECIALS = NANS + [
    0x0000000000000000, 0x8000000000000000,                     # +-0.0
    0x7FF0000000000000, 0xFFF0000000000000,                     # +-inf
    0x0000000000000001, 0x8000000000000001,                     # +-5e-324
    0x0010000000000000, 0x8010000000000000,                     # +-2.2250738585072014e-308, the smallest normal
    0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF,                     # the subnormal just below it
    0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF,                     # +-1.7976931348623157e308
    0x3FF0000000000000, 0xBFF0000000000000,                     # +-1.0
    0x4340000000000000, 0x4340000000000001,                     # 2^53, 2^53 + 2
]
NAN_FREE = [b for b in SPECIALS if not is_nan_bits(b)]
