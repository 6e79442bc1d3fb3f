"""What lies under a NULL.  Arrow leaves the contents of a NULL slot unspecified -- the value under a cleared validity bit, the bytes a Utf8 offset pair
spans for a NULL row -- and pyarrow's `pa.array([.. None ..])` writes 0 and an empty range there: the two values behind which an operator that reads
the slot hides (a NULL added into a SUM, a NULL text measured, a NULL key hashed, a NULL divisor).  This module is the one place that decides what
the tests put there instead.

slot(pool, stratum, seed, i, leaf, column, row, ...) is a pure function of its arguments: the draw of a row is a 64-bit mix of them (no generator
with a state, nothing of plan_corpus' generators is touched), so a failure reproduces without a GPU and every case of the corpus stays what it was.
Each NULL row draws on its own: two NULL rows of a column usually differ.

Two pools per type:
  near  live values of the same column (a NULL that collides with a real key, peer or group), 0, and a live value +- 1 -- each only where it lies
        inside the column's live minimum and maximum, so that the minimum and maximum over ALL slots stay the live ones (minmax_kernel reads every
        slot: the dense routes stay alive).  A column without a live value keeps 0 / ''.
  far   the type's extremes, -1, 0x5555.., 2^40 for the 64-bit types; timestamps one millisecond outside the years 0000 to 9999 and at both ends of
        Int64; NaNs of both signs, both infinities, -0.0, the least subnormal, DBL_MAX; texts that match every pattern of plan_corpus.LIKES, of 17
        and 70 bytes, that do not parse, with slashes, and that are no UTF-8 at all.  0 stays in every numeric pool: the divisor.

Two builders: poisoned_array (an Arrow array over from_buffers: the bitmap, a real null_count, non-empty ranges under NULL Utf8 rows) and
numeric_slots / utf8_slots, from which device_feed_util.device_source builds device columns beside their validity bytes.  unmasked() gives the same slots as LIVE values, for the test
that shows the poison would change the interpreter's answer if anything read it."""
import struct
import zlib

import numpy as np
import pyarrow as pa

import plan_corpus as pc

POOLS = ("near", "far")
_NEG_NAN = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
_POS_NAN = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]

FAR = {
    "Int32": [-2**31, 2**31 - 1, -1, 0x55555555, 0],
    "Int64": [-2**63, 2**63 - 1, -1, 0x5555555555555555, 2**40, 0],
    "UInt64": [0, 2**64 - 1, 0x5555555555555555, 2**40, 2**63],                      # (-1 is the upper extreme)
    "Timestamp": [pc.TS_MAX + 1, pc.TS_MIN - 1, -2**63, 2**63 - 1, 0],
    "Float64": [_POS_NAN, _NEG_NAN, float("inf"), float("-inf"), -0.0, 5e-324, 1.7976931348623157e308, 0.0],
    # one text per pattern of plan_corpus.LIKES ('' is matched by the empty text alone, which is what pyarrow puts there already; '%' by all)
    "Utf8": [b"a far", b"xbx", b"xwx", b"q", "éq far".encode(), "qé".encode(), b"prefix_8 far", b"farz", b"q7", b"a/b/c",
             b"seventeen_bytes__", b"f" * 70, b"12x", b"99999999999999999999", b"\xff\xfe", b"\x80", b"\xe2\x82"],
}
assert len(FAR["Utf8"][10]) == 17 and len(FAR["Utf8"][11]) == 70          # past one 16-byte chunk, past the short-value path


def type_name(t):
    """a field's data_type -> 'Int32' | 'Int64' | 'UInt64' | 'Float64' | 'Utf8' | 'Timestamp'"""
    return "Timestamp" if isinstance(t, dict) or t == "ts" else t


def _mix(x):
    """splitmix64's finaliser over an array of uint64"""
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def draws(pool, stratum, seed, i, leaf, column, rows):
    """one 64-bit draw per row number in `rows`: a function of the arguments alone"""
    head = zlib.crc32(repr((pool, stratum, seed, i, leaf, column)).encode())
    with np.errstate(over="ignore"):
        return _mix(_mix(np.asarray(rows, np.uint64) ^ (np.uint64(head) << np.uint64(32))) + np.uint64(head))


def near_pool(live, ty):
    """the near pool of a column with the live values `live` (no None among them); never outside [min(live), max(live)]"""
    if ty == "Utf8":
        return sorted({v if isinstance(v, bytes) else v.encode() for v in live} | {b""})
    if not live:
        return [0.0 if ty == "Float64" else 0]
    pool = list(dict.fromkeys(live))
    ordered = [v for v in pool if v == v]                        # (a NaN is neither a minimum nor a maximum)
    if not ordered:
        return pool
    lo, hi = min(ordered), max(ordered)
    if ty == "Float64":                                          # (a zero at an end would be a second bit pattern of that end: strictly inside)
        near = ([0.0] if lo < 0.0 < hi else []) + [w for v in ordered[:64] for w in (v - 1.0, v + 1.0) if lo < w < hi]
    else:
        near = [w for w in [0] + [w for v in ordered[:64] for w in (v - 1, v + 1)] if lo <= w <= hi]
    return list(dict.fromkeys(pool + near))


def slots(pool, stratum, seed, i, leaf, column, values, ty):
    """`values` (None = NULL) -> the list of what every slot holds: a live row its value (text as bytes), a NULL row its poison"""
    ty = type_name(ty)
    assert pool in POOLS, pool
    out = [v.encode() if isinstance(v, str) else v for v in values] if ty == "Utf8" else list(values)
    nulls = [k for k, v in enumerate(values) if v is None]
    if not nulls:
        return out
    choices = FAR[ty] if pool == "far" else near_pool([v for v in out if v is not None], ty)
    d = draws(pool, stratum, seed, i, leaf, column, nulls)
    for k, x in zip(nulls, (d % np.uint64(len(choices))).tolist()):
        out[k] = choices[x]
    return out


def slot(pool, stratum, seed, i, leaf, column, row, values, ty):
    """what lies under row `row` of the column (its own value where the row is live)"""
    if values[row] is not None:
        return values[row].encode() if isinstance(values[row], str) else values[row]
    ty = type_name(ty)
    choices = FAR[ty] if pool == "far" else near_pool([v.encode() if isinstance(v, str) else v for v in values if v is not None], ty)
    return choices[int(draws(pool, stratum, seed, i, leaf, column, [row])[0] % np.uint64(len(choices)))]


# ------------------------------------------------------------------ builders
_NP = {"Int32": np.int32, "Int64": np.int64, "UInt64": np.uint64, "Timestamp": np.int64, "Float64": np.float64}
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Timestamp": pa.timestamp("ms"), "Float64": pa.float64(), "Utf8": pa.string()}


def numeric_slots(slot_values, ty):
    """the slots of a numeric column as the numpy array of the type's width (NaN payloads and signs kept)"""
    ty = type_name(ty)
    if ty == "Float64":
        return np.array([struct.unpack("<q", struct.pack("<d", v))[0] for v in slot_values], np.int64).view(np.float64)
    return np.array(slot_values, dtype=_NP[ty])


def utf8_slots(slot_values):
    """-> (int32 offsets, the bytes): every row's range holds its slot, a NULL row's included"""
    off = np.zeros(len(slot_values) + 1, np.int32)
    off[1:] = np.cumsum([len(b) for b in slot_values], dtype=np.int64)
    return off, b"".join(slot_values)


def poisoned_array(slot_values, valid, ty):
    """an Arrow array of type `ty` whose buffers hold `slot_values` and whose bitmap is `valid` (a list of booleans)"""
    ty = type_name(ty)
    n = len(slot_values)
    ok = np.array(valid, bool)
    null_count = int(n - ok.sum())
    bitmap = pa.py_buffer(np.packbits(ok, bitorder="little").tobytes()) if null_count else None
    if ty == "Utf8":
        off, data = utf8_slots(slot_values)
        return pa.StringArray.from_buffers(n, pa.py_buffer(off.tobytes()), pa.py_buffer(data), bitmap, null_count)
    return pa.Array.from_buffers(_PA[ty], n, [bitmap, pa.py_buffer(numeric_slots(slot_values, ty).tobytes())], null_count)


def poisoned_column(pool, key, leaf, column, values, ty, lo=0, hi=None):
    """rows [lo, hi) of a column of case `key` = (stratum, seed, i) as an Arrow array; a row's poison does not depend on the cut"""
    s = slots(pool, key[0], key[1], key[2], leaf, column, values, ty)
    return poisoned_array(s[lo:hi], [v is not None for v in values[lo:hi]], ty)


def unmasked(pool, key, leaf, column, values, ty):
    """the column with every NULL replaced by its poison AS A LIVE VALUE, in the interpreter's types (text as str: bytes that are no UTF-8 become
    U+FFFD, the nearest thing a str can hold)"""
    s = slots(pool, key[0], key[1], key[2], leaf, column, values, ty)
    return [v.decode("utf-8", "replace") if isinstance(v, bytes) else v for v in s]
