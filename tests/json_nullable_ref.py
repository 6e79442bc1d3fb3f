"""The reference of flockgpu_json_lines_decode_nullable's contract (json.hip, A-JSONN1..7): tests/json_ref.py's from-scratch decoder with NULLs, optional
members and the encoders' six types.  What carries over (lines, strings, dropped members, schema integers, the error order) is json_ref's own code, used
as it is; what is new -- null, absence, UInt64, Timestamp(ms), Float64 -- is written here, on Python integers alone: nothing goes through json or float().
tests/test_json_nullable_reference.py holds it against json.loads and float() line by line.

    decode(text, fields) -> ({name: np.ndarray | oracle.Utf8}, {name: uint8 validity of every NULLABLE field}, {name: null count})
                                                                      fields = [(name, type)] | [(name, type, nullable)], nullable defaults to True
                                                                      type: "int32" | "int64" | "uint64" | "float64" | "timestamp_ms" | "utf8"
    JsonError(line, code, field)                                      line: 1-based, the FIRST offending line; .status, .message

A NULL is validity 0 and value 0; a Utf8 NULL is a value of length 0.  uint64 columns are np.uint64, float64 columns np.float64."""
import numpy as np

import json_ref
import oracle
from json_ref import WS, _Bad, _digits, _fraction_exponent, _integer, _skip, _string, _ws, lines_of

TYPES = ("int32", "int64", "uint64", "float64", "timestamp_ms", "utf8")
STATUS = dict(json_ref.STATUS, float="unsupported")
# "float" names the field: MESSAGES["float"] % name
MESSAGES = dict(json_ref.MESSAGES,
                float="field '%s': Float64 outside the exactly convertible range (a significand of at most 2^53, a decimal exponent in [-22, 22])")
MAX_SIGNIFICAND, MAX_POW10 = 1 << 53, 22
DELIMITERS = b",} \t\r\n"


class JsonError(Exception):
    def __init__(self, line, code, field=None):
        self.line, self.code, self.field, self.status = line, code, field, STATUS[code]
        self.message = MESSAGES[code] % field if code == "float" else MESSAGES[code]
        super().__init__("line %d: %s" % (line, self.message))


def normalise(fields):
    return [(f[0], f[1], bool(f[2]) if len(f) > 2 else True) for f in fields]


def exact_f64(token):
    """A JSON number's text -> the double, where ONE IEEE operation on exact operands gives it (csv.hpp A-CSV5); None outside that range.  Integer
    arithmetic up to the last step: int -> float and int / int are correctly rounded in Python."""
    neg = token[:1] == b"-"
    mantissa, _, exponent = token[neg:].replace(b"E", b"e").partition(b"e")
    whole, _, frac = mantissa.partition(b".")
    w = int(whole + frac)
    if w == 0:
        return -0.0 if neg else 0.0
    e = (int(exponent) if exponent else 0) - len(frac)
    while w % 10 == 0:
        w //= 10
        e += 1
    if w > MAX_SIGNIFICAND or not -MAX_POW10 <= e <= MAX_POW10:
        return None
    v = float(w * 10 ** e) if e >= 0 else w / 10 ** -e
    return -v if neg else v


def _float(s, p, name):
    """A Float64 member at s[p] -> (position after it, value): the grammar, what follows the number, then the range."""
    b = p
    if s[p] == ord("-"):
        p += 1
    if p >= len(s) or s[p] not in json_ref.DIGITS:
        raise _Bad("malformed")                         # no number: a string, true, +1, .5, nan, Infinity
    q = _digits(s, p)
    if s[p] == ord("0") and q > p + 1:
        raise _Bad("malformed")                         # leading zeros
    q = _fraction_exponent(s, q)                        # "1.", "1e": malformed
    if q < len(s) and s[q] not in DELIMITERS:
        raise _Bad("malformed")
    v = exact_f64(s[b:q])
    if v is None:
        raise _Bad("float", name)
    return q, v


def _uint64(s, p):
    neg = s[p] == ord("-")
    q, v = _integer(s, p, 4096)                         # json_ref's digits, tail and fraction / exponent checks; no range of its own at this width
    if neg or v >= 1 << 64:
        raise _Bad("range")                             # "-0" as well
    return q, v


def parse_line(line, fields):
    """One line (without its newline) -> {name: int | float | bytes | None}; None is a NULL."""
    fields = normalise(fields)
    s = bytes(line).strip(WS)
    if not s:
        raise _Bad("blank")
    if s[0] != ord("{"):
        raise _Bad("malformed")
    types = {n: (t, nl) for n, t, nl in fields}
    row = {}
    p = _ws(s, 1)
    if p < len(s) and s[p] == ord("}"):
        p += 1
    else:
        while True:
            p = _ws(s, p)
            if p >= len(s) or s[p] != 0x22:
                raise _Bad("malformed")
            key_at = p
            p, _, esc = _string(s, p)
            if esc:
                raise _Bad("key_escape")
            key = s[key_at + 1:p - 1].decode("latin-1")
            p = _ws(s, p)
            if p >= len(s) or s[p] != ord(":"):
                raise _Bad("malformed")
            p = _ws(s, p + 1)
            if p >= len(s):
                raise _Bad("malformed")
            t, nullable = types.get(key, (None, False))
            if t is None:
                p = _skip(s, p, 0)
            elif nullable and s[p] == ord("n"):
                if s[p:p + 4] != b"null":
                    raise _Bad("malformed")             # nul
                p, row[key] = p + 4, None               # (nullx fails at the delimiter below)
            elif t == "utf8":
                if s[p] != 0x22:
                    raise _Bad("malformed")
                p, row[key], _ = _string(s, p)
            elif t == "float64":
                p, row[key] = _float(s, p, key)
            elif t == "uint64":
                p, row[key] = _uint64(s, p)
            else:
                p, row[key] = _integer(s, p, 32 if t == "int32" else 64)
            p = _ws(s, p)
            if p >= len(s):
                raise _Bad("malformed")
            if s[p] == ord(","):
                p += 1
                continue
            if s[p] == ord("}"):
                p += 1
                break
            raise _Bad("malformed")
    if p != len(s):
        raise _Bad("malformed")                         # bytes behind the object
    for name, _, nullable in fields:
        if name not in row:
            if not nullable:
                raise _Bad("missing")
            row[name] = None
    return row


DTYPES = {"int32": np.int32, "int64": np.int64, "timestamp_ms": np.int64, "uint64": np.uint64, "float64": np.float64}


def decode(text, fields):
    fields = normalise(fields)
    if len({n for n, _, _ in fields}) != len(fields):
        raise ValueError("json_nullable_ref: the field names are distinct")
    rows = []
    for i, line in enumerate(lines_of(text)):
        try:
            rows.append(parse_line(line, fields))
        except _Bad as e:
            raise JsonError(i + 1, *e.args) from None
    cols, valid, nulls = {}, {}, {}
    for name, t, nullable in fields:
        vals = [r[name] for r in rows]
        if nullable:
            valid[name] = np.array([v is not None for v in vals], np.uint8)
        nulls[name] = sum(v is None for v in vals)
        if t == "utf8":
            vals = [b"" if v is None else v for v in vals]
            off = np.zeros(len(vals) + 1, np.int32)
            if vals:
                np.cumsum([len(v) for v in vals], out=off[1:])
            cols[name] = oracle.Utf8(off, np.frombuffer(b"".join(vals), np.uint8).copy())
        else:
            cols[name] = np.array([0 if v is None else v for v in vals], DTYPES[t])
    return cols, valid, nulls
