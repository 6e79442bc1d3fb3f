"""Reference encoder for flockgpu_json_lines_encode / flockgpu_csv_encode (flock_amd/csrc/textenc.hpp A-ENC1..10) in plain Python: the rules restated byte
by byte and nothing cleverer -- no json or csv module (tests/test_text_encode_reference.py checks it AGAINST json.dumps, csv_ref.decode and csv.reader).

    columns   [(name, "int32" | "int64" | "uint64" | "timestamp_ms" | "utf8", numpy array | Utf8(offsets, data))]; a uint64 column may come as the int64
              array of its bits (what the device takes);
    valid     {name: uint8[rows]}, 1 = not NULL; a column without an entry has no NULLs.
json_lines(columns, valid) and csv_text(columns, valid, delimiter, has_header) return the text's bytes; EncodeError(status, record, column) is the refusal
the device gives for the same input (record 1-based with the header counted, None before any row is looked at)."""
from collections import namedtuple

import numpy as np

Utf8 = namedtuple("Utf8", "offsets data")
TYPES = ("int32", "int64", "uint64", "timestamp_ms", "utf8")
TS_MIN = -62167219200000     # 0000-01-01 00:00:00
TS_MAX = 253402300799999     # 9999-12-31 23:59:59.999
MAX_COLUMNS, MAX_NAME = 64, 31
SHORT = {0x22: b'\\"', 0x5C: b"\\\\", 0x08: b"\\b", 0x0C: b"\\f", 0x0A: b"\\n", 0x0D: b"\\r", 0x09: b"\\t"}


class EncodeError(Exception):
    def __init__(self, status, record=None, column=None):
        self.status, self.record, self.column = status, record, column
        super().__init__("%s: record %s column %s" % (status, record, column))


def utf8_of(values):
    """A list of bytes -> Utf8(offsets int32[rows + 1], data uint8[...])."""
    off = np.zeros(len(values) + 1, np.int32)
    off[1:] = np.cumsum([len(v) for v in values], dtype=np.int64)
    return Utf8(off, np.frombuffer(b"".join(values), np.uint8).copy())


def strings_of(col):
    data = bytes(np.asarray(col.data, np.uint8))
    return [data[col.offsets[i]:col.offsets[i + 1]] for i in range(len(col.offsets) - 1)]


def json_string(raw):
    out = bytearray(b'"')
    for b in raw:
        if b in SHORT:
            out += SHORT[b]
        elif b < 0x20:
            out += b"\\u00" + b"0123456789abcdef"[b >> 4:(b >> 4) + 1] + b"0123456789abcdef"[b & 15:(b & 15) + 1]
        else:
            out.append(b)
    out += b'"'
    return bytes(out)


def csv_string(raw, delim):
    if raw == b"" or any(b in (delim, 0x22, 0x0A, 0x0D) for b in raw):
        return b'"' + raw.replace(b'"', b'""') + b'"'
    return raw


def days_to_civil(days):
    """Days since 1970-01-01 -> (year, month, day) of the proleptic Gregorian calendar, by walking: 400-year cycles, then years, then months."""
    days += 719528                      # days since 0000-01-01
    year = 400 * (days // 146097)
    days %= 146097
    leap = lambda y: y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)
    while days >= (366 if leap(year) else 365):
        days -= 366 if leap(year) else 365
        year += 1
    month = 1
    for n in (31, 29 if leap(year) else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31):
        if days < n:
            break
        days -= n
        month += 1
    return year, month, days + 1


def timestamp_text(ms):
    days, in_day = divmod(ms, 86400000)         # (floor division: times before 1970 round towards minus infinity)
    y, mo, d = days_to_civil(days)
    s, milli = divmod(in_day, 1000)
    text = "%04d-%02d-%02d %02d:%02d:%02d" % (y, mo, d, s // 3600, s // 60 % 60, s % 60)
    return (text + (".%03d" % milli if milli else "")).encode()


def _int(t, v):
    v = int(v)
    return v % 2**64 if t == "uint64" else v


def _check(columns, delimiter=None):
    if not columns:
        raise EncodeError("invalid")
    if len(columns) > MAX_COLUMNS:
        raise EncodeError("unsupported", None, MAX_COLUMNS)
    if delimiter is not None and (len(delimiter) != 1 or delimiter[0] >= 0x80 or delimiter[0] in (0x22, 0x0D, 0x0A)):
        raise EncodeError("invalid")
    for c, (name, t, _) in enumerate(columns):
        key = name.encode() if isinstance(name, str) else name
        if not 1 <= len(key) <= MAX_NAME or t == "float64":
            raise EncodeError("unsupported", None, c)
        if t not in TYPES:
            raise EncodeError("invalid", None, c)


def _rows(columns):
    _, t, col = columns[0]
    return len(col.offsets) - 1 if t == "utf8" else len(col)


def _cells(columns, valid, fmt, delim=None, header=0):
    """Per column the list of its values' texts (None = NULL)."""
    valid = valid or {}
    out = []
    for c, (name, t, col) in enumerate(columns):
        ok = valid.get(name)
        if t == "utf8":
            vals = [json_string(s) if fmt == "json" else csv_string(s, delim) for s in strings_of(col)]
        elif t == "timestamp_ms" and fmt == "csv":
            vals = [None if (ok is not None and not ok[i]) else int(v) for i, v in enumerate(col)]
            vals = [v if v is None else (timestamp_text(v) if TS_MIN <= v <= TS_MAX else ("bad", i)) for i, v in enumerate(vals)]
        else:
            vals = [str(_int(t, v)).encode() for v in col]
        if ok is not None:
            vals = [v if ok[i] else None for i, v in enumerate(vals)]
        out.append(vals)
    bad = [(v[1], c) for c, vals in enumerate(out) for v in vals if isinstance(v, tuple)]
    if bad:                              # the first such ROW, and in it the first column
        row, c = min(bad)
        raise EncodeError("invalid", row + 1 + header, c)
    return out


def json_lines(columns, valid=None):
    _check(columns)
    keys = [json_string(name.encode() if isinstance(name, str) else name) for name, _, _ in columns]
    cells = _cells(columns, valid, "json")
    out = bytearray()
    for i in range(_rows(columns)):
        out += b"{" + b",".join(k + b":" + (b"null" if col[i] is None else col[i]) for k, col in zip(keys, cells)) + b"}\n"
    if len(out) >= 2**31 - 16:
        raise EncodeError("unsupported")
    return bytes(out)


def csv_text(columns, valid=None, delimiter=b",", has_header=True):
    _check(columns, delimiter)
    cells = _cells(columns, valid, "csv", delimiter[0], 1 if has_header else 0)
    out = bytearray()
    if has_header:
        out += delimiter.join(csv_string(name.encode() if isinstance(name, str) else name, delimiter[0]) for name, _, _ in columns) + b"\n"
    for i in range(_rows(columns)):
        record = delimiter.join(b"" if col[i] is None else col[i] for col in cells)
        out += (record or b'""') + b"\n"
    if len(out) >= 2**31 - 16:
        raise EncodeError("unsupported")
    return bytes(out)
