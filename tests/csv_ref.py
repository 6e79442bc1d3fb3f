"""Reference decoder for flockgpu_csv_decode (flock_amd/csrc/csv.hpp A-CSV1..7) in plain Python: ONE explicit state machine over the bytes of the text,
in stream order, with the typed parsing and every error case -- not a wrapper around the csv module (tests/test_csv_reference.py checks it AGAINST
csv.reader(strict=True) and pyarrow.csv.read_csv on well-formed text).  Integers and timestamps go through parse_text_ref.py, the reference of
textnum.hpp; the Float64 rule of A-CSV5 and the nine-digit fraction of A-CSV4 are restated here.

decode(text, fields, delimiter=b",", has_header=True) -> (columns, validity, rows):
    fields     [(name, "int32" | "int64" | "uint64" | "float64" | "timestamp_ms" | "utf8" | None)], one per column of the file, None = skip;
    columns    {name: numpy array (int32 / int64 / uint64 / float64; NULL slots hold 0) | Utf8(offsets int32[rows + 1], data uint8[...])};
    validity   {name: uint8[rows]} for EVERY numeric column (1 = not NULL); null_count is its zeros.
A failure raises CsvError(status, record, column, code): status "unsupported" | "invalid", record 1-based with the header counted, and -- first in
stream order -- the same one the device reports (A-CSV7)."""
import re
from collections import namedtuple

import numpy as np

from parse_text_ref import parse_int, parse_ts

Utf8 = namedtuple("Utf8", "offsets data")
TYPES = ("int32", "int64", "uint64", "float64", "timestamp_ms", "utf8")
TYPE_NAMES = {"int32": "Int32", "int64": "Int64", "uint64": "UInt64", "float64": "Float64", "timestamp_ms": "Timestamp(ms)", "utf8": "Utf8"}
DTYPES = {"int32": np.int32, "int64": np.int64, "uint64": np.uint64, "float64": np.float64, "timestamp_ms": np.int64}
UNSUPPORTED = ("blank", "bare_cr", "float")      # every other code is "invalid"

_FLOAT = re.compile(r"([+-]?)([0-9]+)(?:\.([0-9]+))?(?:[eE]([+-]?[0-9]+))?")
_TS_LONG = re.compile(r".{19}\.[0-9]{4,9}", re.S)


class CsvError(Exception):
    def __init__(self, record, column, code):
        self.status = "unsupported" if code in UNSUPPORTED else "invalid"
        self.record, self.column, self.code = record, column, code
        super().__init__("record %d column %d: %s" % (record, column, code))


def parse_float(s):
    """A-CSV5: the double nearest to the text where one IEEE operation gives it, None everywhere else."""
    m = _FLOAT.fullmatch(s)
    if not m:
        return None
    sign, whole, frac, exp = m.group(1), m.group(2), m.group(3) or "", int(m.group(4) or "0")
    w, e = int(whole + frac), exp - len(frac)
    if w == 0:
        return -0.0 if sign == "-" else 0.0
    while w % 10 == 0:
        w, e = w // 10, e + 1
    if w > 2**53 or not -22 <= e <= 22:
        return None
    v = float(w) * float(10**e) if e >= 0 else float(w) / float(10**-e)     # (w and 10^|e| are exact doubles: one rounding)
    return -v if sign == "-" else v


def parse_timestamp(s):
    """A-CSV4: textnum's Timestamp(ms); four to nine fraction digits parse as their first three."""
    return parse_ts(s[:23]) if _TS_LONG.fullmatch(s) else parse_ts(s)


def parse_value(raw, ty):
    s = raw.decode("latin-1")       # (one character per byte: nothing above 0x7F is part of any number)
    if ty == "float64":
        return parse_float(s)
    if ty == "timestamp_ms":
        return parse_timestamp(s)
    return parse_int(s, TYPE_NAMES[ty])


def records(text, delimiter=b","):
    """The state machine: yields (record number, [field bytes after unquoting, ...]) in stream order; structural failures raise CsvError.
    on_field (decode) sees every field the moment it is complete, so that the first failure in stream order wins."""
    return _machine(text, delimiter, None)


def _machine(text, delimiter, on_field):
    d = delimiter[0]
    QUOTE, CR, LF = 0x22, 0x0D, 0x0A
    START, UNQUOTED, QUOTED, QUOTE_IN_QUOTED = range(4)     # QUOTE_IN_QUOTED: a '"' inside a quoted field -- the closing one, or half of '""'
    n = len(text)
    record, fields, cur, state, rec_start, i = 1, [], bytearray(), START, 0, 0

    def end_field(more):                # more: a delimiter ended it, another field follows
        fields.append(bytes(cur))
        if on_field:
            on_field(record, len(fields) - 1, fields[-1], more)
        cur.clear()

    while i <= n:
        c = text[i] if i < n else -1        # -1: the end of the text
        if state == QUOTED:
            if c == -1:
                raise CsvError(record, len(fields), "open_quote")
            if c == QUOTE:
                state = QUOTE_IN_QUOTED
            else:
                cur.append(c)
            i += 1
            continue
        if state == QUOTE_IN_QUOTED and c == QUOTE:
            cur.append(QUOTE)
            state = QUOTED
            i += 1
            continue
        # outside quotes: a terminator?
        crlf = c == CR and i + 1 < n and text[i + 1] == LF
        if c == LF or crlf or c == -1:
            if c == -1 and i == rec_start:
                break                       # the text ended with a terminator (or is empty)
            if i == rec_start:
                raise CsvError(record, 0, "blank")
            end_field(False)
            yield record, fields
            record, fields, state = record + 1, [], START
            i += 2 if crlf else 1
            rec_start = i
            continue
        if state == QUOTE_IN_QUOTED:        # the quote was the closing one: only a delimiter may follow
            if c != d:
                raise CsvError(record, len(fields), "after_quote")
            end_field(True)
            state = START
        elif c == d:
            end_field(True)
            state = START
        elif c == QUOTE:
            if state != START:
                raise CsvError(record, len(fields), "stray_quote")
            state = QUOTED
        elif c == CR:
            raise CsvError(record, len(fields), "bare_cr")
        else:
            cur.append(c)
            state = UNQUOTED
        i += 1


# The fixtures under tests/golden/csv (data files of the reference's own tests) with their real schemas: (file, delimiter, has_header, fields).  A '.tbl'
# line ends in '|': one more skipped column.  lineitem's ship and commit dates are read as Timestamp(ms), its receipt date as Utf8.
# citibike_sample.csv: of the first 256 records of JC-202011-citibike-tripdata.csv the 214 that A-CSV5's exact Float64 range covers; the other 42 hold a
# station latitude of 17 significant digits ('40.722103786686034' is more than 2^53 as a significand), which the decoder refuses by design.
def _f(spec):
    return [(name, {"i": "int32", "l": "int64", "u": "uint64", "d": "float64", "t": "timestamp_ms", "s": "utf8", "-": None}[k]) for k, name in
            (x.split(":") for x in spec.split())]


_LINEITEM = _f("l:l_orderkey l:l_partkey l:l_suppkey i:l_linenumber d:l_quantity d:l_extendedprice d:l_discount d:l_tax s:l_returnflag s:l_linestatus "
               "t:l_shipdate t:l_commitdate s:l_receiptdate s:l_shipinstruct s:l_shipmode s:l_comment -:end")
FIXTURES = {
    "uk_cities": ("uk_cities_with_headers.csv", b",", True, _f("s:city d:lat d:lng")),
    "citibike": ("citibike_sample.csv", b",", True,
                 _f("i:tripduration t:starttime t:stoptime i:start_station_id s:start_station_name d:start_station_latitude d:start_station_longitude "
                    "i:end_station_id s:end_station_name d:end_station_latitude d:end_station_longitude l:bikeid s:usertype i:birth_year i:gender")),
    "customer": ("tpch/customer.tbl", b"|", False, _f("l:c_custkey s:c_name s:c_address l:c_nationkey s:c_phone d:c_acctbal s:c_mktsegment s:c_comment -:end")),
    "lineitem0": ("tpch/lineitem_partition0.tbl", b"|", False, _LINEITEM),
    "lineitem1": ("tpch/lineitem_partition1.tbl", b"|", False, _LINEITEM),
    "nation": ("tpch/nation.tbl", b"|", False, _f("i:n_nationkey s:n_name i:n_regionkey s:n_comment -:end")),
    "orders": ("tpch/orders.tbl", b"|", False,
               _f("l:o_orderkey l:o_custkey s:o_orderstatus d:o_totalprice t:o_orderdate s:o_orderpriority s:o_clerk i:o_shippriority s:o_comment -:end")),
    "part": ("tpch/part.tbl", b"|", False, _f("l:p_partkey s:p_name s:p_mfgr s:p_brand s:p_type i:p_size s:p_container d:p_retailprice s:p_comment -:end")),
    "partsupp": ("tpch/partsupp.tbl", b"|", False, _f("l:ps_partkey l:ps_suppkey i:ps_availqty d:ps_supplycost s:ps_comment -:end")),
    "region": ("tpch/region.tbl", b"|", False, _f("i:r_regionkey s:r_name s:r_comment -:end")),
    "supplier": ("tpch/supplier.tbl", b"|", False, _f("l:s_suppkey s:s_name s:s_address i:s_nationkey s:s_phone d:s_acctbal s:s_comment -:end")),
}


def fixture(name):
    """(text bytes, delimiter, has_header, fields) of one fixture."""
    import os
    path, delim, header, fields = FIXTURES[name]
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "csv", path), "rb") as f:
        return f.read(), delim, header, fields


def decode(text, fields, delimiter=b",", has_header=True):
    text = bytes(text)
    n_fields = len(fields)
    values = [[] for _ in fields]
    first = 2 if has_header else 1

    def on_field(record, column, raw, more):
        if record < first:
            return
        ty = fields[column][1]
        if ty is None:
            pass
        elif ty == "utf8":
            values[column].append(raw)
        elif raw == b"":
            values[column].append(None)
        else:
            v = parse_value(raw, ty)
            if v is None:
                raise CsvError(record, column, "float" if ty == "float64" else "value")
            values[column].append(v)
        if more and column == n_fields - 1:
            raise CsvError(record, column, "many_fields")

    rows = 0
    for record, got in _machine(text, delimiter, on_field):
        if record < first:
            continue
        if len(got) < n_fields:
            raise CsvError(record, len(got) - 1, "few_fields")
        rows += 1
    cols, valid = {}, {}
    for (name, ty), v in zip(fields, values):
        if ty is None:
            continue
        if ty == "utf8":
            off = np.zeros(rows + 1, np.int32)
            off[1:] = np.cumsum([len(b) for b in v], dtype=np.int64)
            cols[name] = Utf8(off, np.frombuffer(b"".join(v), np.uint8))
        else:
            cols[name] = np.array([0 if x is None else x for x in v], dtype=DTYPES[ty])
            valid[name] = np.array([x is not None for x in v], dtype=np.uint8)
    return cols, valid, rows
