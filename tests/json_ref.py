"""The reference of flockgpu_json_lines_decode's contract (json.hip, A-JSON1..9): a from-scratch recursive-descent decoder of newline-delimited
JSON objects into columns.  It builds nothing on Python's json module -- tests/test_json_reference.py holds it against json.loads line by line.

    decode(text, fields) -> {name: np.ndarray | oracle.Utf8}          fields = [(name, "int32" | "int64" | "utf8")]
    JsonError(line, status, code)                                     line: 1-based, the FIRST offending line; status: "invalid" | "unsupported"

The codes are the decoder's seven (json.hip kErr*), MESSAGES their wording in the library's error text."""
import numpy as np

import oracle

MAX_DEPTH = 64                    # json.hip kMaxDepth: brackets nested inside a member that is not in the schema
WS = b" \t\r\n"
STATUS = {"malformed": "invalid", "number": "unsupported", "missing": "invalid", "blank": "unsupported", "key_escape": "unsupported",
          "range": "invalid", "depth": "unsupported"}
MESSAGES = {"malformed": "malformed JSON", "number": "number with a fraction / exponent (integer literal expected)", "missing": "a schema field is missing",
            "blank": "blank line", "key_escape": "escape sequence in a key", "range": "integer out of range",
            "depth": "brackets nested more than 64 deep in a member that is not in the schema"}
SINGLE = {ord('"'): 0x22, ord("\\"): 0x5C, ord("/"): 0x2F, ord("b"): 8, ord("f"): 12, ord("n"): 10, ord("r"): 13, ord("t"): 9}
DIGITS = b"0123456789"


class JsonError(Exception):
    def __init__(self, line, code):
        super().__init__("line %d: %s" % (line, MESSAGES[code]))
        self.line, self.code, self.status = line, code, STATUS[code]


class _Bad(Exception):
    """One line's failure: its code."""


def _ws(s, p):
    while p < len(s) and s[p] in WS:
        p += 1
    return p


def _hex4(s, p):
    """The value of the four hex digits at s[p: p + 4] (either case); they are all there and all hex, or the line is malformed."""
    if p + 4 > len(s):
        raise _Bad("malformed")
    v = 0
    for c in s[p:p + 4]:
        if c in DIGITS:
            d = c - 48
        elif 97 <= c <= 102:
            d = c - 87
        elif 65 <= c <= 70:
            d = c - 55
        else:
            raise _Bad("malformed")
        v = v * 16 + d
    return v


def _string(s, p):
    """s[p] is the opening quote.  -> (position after the closing quote, the value's bytes after unescaping, whether it held a backslash)."""
    p += 1
    out, esc = bytearray(), False
    while p < len(s):
        c = s[p]
        if c == 0x22:
            return p + 1, bytes(out), esc
        if c < 0x20:
            raise _Bad("malformed")                     # a raw control byte
        if c != 0x5C:
            out.append(c)                               # bytes >= 0x80 included, as they are (A-JSON7)
            p += 1
            continue
        esc = True
        if p + 1 >= len(s):
            raise _Bad("malformed")
        d = s[p + 1]
        if d in SINGLE:
            out.append(SINGLE[d])
            p += 2
            continue
        if d != ord("u"):
            raise _Bad("malformed")
        cp = _hex4(s, p + 2)
        p += 6
        if 0xDC00 <= cp <= 0xDFFF:
            raise _Bad("malformed")                     # a low surrogate on its own
        if 0xD800 <= cp < 0xDC00:
            if s[p:p + 2] != b"\\u":
                raise _Bad("malformed")
            lo = _hex4(s, p + 2)
            if not 0xDC00 <= lo <= 0xDFFF:
                raise _Bad("malformed")
            p += 6
            cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00)
        if cp < 0x80:
            out.append(cp)
        elif cp < 0x800:
            out += bytes([0xC0 | cp >> 6, 0x80 | cp & 0x3F])
        elif cp < 0x10000:
            out += bytes([0xE0 | cp >> 12, 0x80 | cp >> 6 & 0x3F, 0x80 | cp & 0x3F])
        else:
            out += bytes([0xF0 | cp >> 18, 0x80 | cp >> 12 & 0x3F, 0x80 | cp >> 6 & 0x3F, 0x80 | cp & 0x3F])
    raise _Bad("malformed")                             # no closing quote


def _digits(s, p):
    while p < len(s) and s[p] in DIGITS:
        p += 1
    return p


def _fraction_exponent(s, p):
    """(\\.[0-9]+)?([eE][+-]?[0-9]+)? at p -> the position after them."""
    if p < len(s) and s[p] == ord("."):
        q = _digits(s, p + 1)
        if q == p + 1:
            raise _Bad("malformed")
        p = q
    if p < len(s) and s[p] in b"eE":
        p += 1
        if p < len(s) and s[p] in b"+-":
            p += 1
        q = _digits(s, p)
        if q == p:
            raise _Bad("malformed")
        p = q
    return p


def _skip(s, p, depth):
    """Any value at s[p] (a member that is not in the schema), checked in full -> the position after it.  depth: brackets already open."""
    if p >= len(s):
        raise _Bad("malformed")
    c = s[p]
    if c == 0x22:
        return _string(s, p)[0]
    if c in b"{[":
        if depth == MAX_DEPTH:
            raise _Bad("depth")
        obj, close = c == ord("{"), ord("}") if c == ord("{") else ord("]")
        p = _ws(s, p + 1)
        if p < len(s) and s[p] == close:
            return p + 1
        while True:
            p = _ws(s, p)
            if obj:
                if p >= len(s) or s[p] != 0x22:
                    raise _Bad("malformed")
                p = _ws(s, _string(s, p)[0])            # a key INSIDE a dropped value is a plain string
                if p >= len(s) or s[p] != ord(":"):
                    raise _Bad("malformed")
                p = _ws(s, p + 1)
            p = _ws(s, _skip(s, p, depth + 1))
            if p >= len(s):
                raise _Bad("malformed")
            if s[p] == ord(","):
                p += 1
                continue
            if s[p] == close:
                return p + 1
            raise _Bad("malformed")
    for lit in (b"true", b"false", b"null"):
        if c == lit[0]:
            if s[p:p + len(lit)] != lit:
                raise _Bad("malformed")
            return p + len(lit)
    if c == ord("-"):
        p += 1
    if p >= len(s) or s[p] not in DIGITS:
        raise _Bad("malformed")
    p = p + 1 if s[p] == ord("0") else _digits(s, p)
    return _fraction_exponent(s, p)


def _integer(s, p, bits):
    """A schema integer at s[p] -> (position after it, value).  A-JSON8: the digits to their end, then the tail, then the range."""
    neg = s[p] == ord("-")
    p += neg
    if p >= len(s) or s[p] not in DIGITS:
        raise _Bad("malformed")                         # no number at all: a string, true, null, a lone '-'
    q = _digits(s, p)
    if s[p] == ord("0") and q > p + 1:
        raise _Bad("malformed")                         # leading zeros
    if q < len(s) and s[q] not in b",} \t\r\n":
        try:
            if s[q] not in b".eE":
                raise _Bad("malformed")
            r = _fraction_exponent(s, q)
            if r < len(s) and s[r] not in b",} \t\r\n":
                raise _Bad("malformed")
        except _Bad:
            raise _Bad("malformed") from None
        raise _Bad("number")                            # well formed, only no integer literal
    v = 0
    for c in s[p:q]:
        v = v * 10 + (c - 48)
    v = -v if neg else v
    if not -(1 << bits - 1) <= v < (1 << bits - 1):
        raise _Bad("range")
    return q, v


def parse_line(line, fields):
    """One line (without its newline) -> {name: int | bytes}."""
    s = bytes(line).strip(WS)
    if not s:
        raise _Bad("blank")
    if s[0] != ord("{"):
        raise _Bad("malformed")
    types = dict(fields)
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
            p, key, esc = _string(s, p)
            if esc:
                raise _Bad("key_escape")
            key = s[key_at + 1:p - 1]
            p = _ws(s, p)
            if p >= len(s) or s[p] != ord(":"):
                raise _Bad("malformed")
            p = _ws(s, p + 1)
            if p >= len(s):
                raise _Bad("malformed")
            t = types.get(key.decode("latin-1"))        # (names are ASCII in every schema here; the comparison is byte for byte)
            if t is None:
                p = _skip(s, p, 0)
            elif t == "utf8":
                if s[p] != 0x22:
                    raise _Bad("malformed")
                p, row[key], _ = _string(s, p)
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
    if len(row) != len(types):
        raise _Bad("missing")
    return {k.decode("latin-1"): v for k, v in row.items()}


def lines_of(text):
    """A-JSON1: every 0x0A ends a line; what follows the last one, if anything does, is a line too."""
    lines = bytes(text).split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def decode(text, fields):
    rows = []
    for i, line in enumerate(lines_of(text)):
        try:
            rows.append(parse_line(line, fields))
        except _Bad as e:
            raise JsonError(i + 1, e.args[0]) from None
    out = {}
    for name, t in fields:
        if t == "utf8":
            vals = [r[name] for r in rows]
            off = np.zeros(len(vals) + 1, np.int32)
            if vals:
                np.cumsum([len(v) for v in vals], out=off[1:])
            out[name] = oracle.Utf8(off, np.frombuffer(b"".join(vals), np.uint8).copy())
        else:
            out[name] = np.array([r[name] for r in rows], np.int32 if t == "int32" else np.int64)
    return out
