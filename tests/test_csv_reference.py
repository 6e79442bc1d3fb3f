"""tests/csv_ref.py, the reference the GPU tests compare flockgpu_csv_decode with (csv.hpp A-CSV1..7), checked on the CPU: against hand-worked records
(every quote rule, CRLF, an embedded newline, a trailing delimiter column, NULLs, each error with its record number), against Python's
csv.reader(strict=True) and pyarrow.csv.read_csv on a seeded well-formed corpus, its Float64 against float() in both directions, and on the fixtures
under tests/golden/csv, of which not one field may be refused.

What the corpus leaves out, because the other two readers differ there ON PURPOSE or by their own rules:
  * a leading '+' on a number (pyarrow refuses it; A-TN1 takes it) and 'T' / fraction forms of timestamps other than 'YYYY-MM-DD' and
    'YYYY-MM-DD hh:mm:ss[.fff]' (pyarrow's ISO-8601 forms differ; year 0000 is refused there) -- both covered by tests/test_plan_parse_text.py's corpus;
  * a quoted EMPTY numeric field (NULL here; pyarrow's quoted_strings_can_be_null speaks of strings) -- hand-worked below;
  * a bare '\\r' inside an UNQUOTED field and blank lines (refused here; csv.reader and pyarrow take or skip them) -- hand-worked below;
  * Float64 texts outside the exact range (refused here, converted by both others) -- the float() test below covers the boundary;
  * malformed quoting of any kind (strict=True raises, pyarrow raises or guesses) -- hand-worked below."""
import csv
import io
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import csv_ref
from csv_ref import CsvError, decode, parse_float, parse_timestamp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, L, U, D, T, S = "int32", "int64", "uint64", "float64", "timestamp_ms", "utf8"


def _strings(col):
    return [bytes(col.data[col.offsets[i]:col.offsets[i + 1]]) for i in range(len(col.offsets) - 1)]


def _fields(*types):
    return [("c%d" % i, t) for i, t in enumerate(types)]


# ---- hand-worked records -------------------------------------------------------------------------------------------------------------------------------------
def test_quote_rules():
    text = (b'h1,h2,h3\n'
            b'plain,"quoted",3\n'
            b'"with, delimiter","say ""hi""",-4\n'
            b'"line one\nline two","cr\rinside\r\nand crlf",5\n'
            b'"""","""""",6\n'
            b'mid space,,7')
    cols, valid, rows = decode(text, _fields(S, S, I))
    assert rows == 5
    assert _strings(cols["c0"]) == [b"plain", b"with, delimiter", b"line one\nline two", b'"', b"mid space"]
    assert _strings(cols["c1"]) == [b"quoted", b'say "hi"', b"cr\rinside\r\nand crlf", b'""', b""]
    assert cols["c2"].tolist() == [3, -4, 5, 6, 7] and valid["c2"].tolist() == [1] * 5


def test_crlf_and_missing_final_terminator():
    for text in (b"a,b\r\n1,x\r\n2,y\r\n", b"a,b\r\n1,x\r\n2,y", b"a,b\n1,x\r\n2,y\n"):
        cols, _, rows = decode(text, _fields(I, S))
        assert rows == 2 and cols["c0"].tolist() == [1, 2] and _strings(cols["c1"]) == [b"x", b"y"]
    assert decode(b"", _fields(I))[2] == 0 and decode(b"", _fields(I), has_header=False)[2] == 0
    assert decode(b"only,header\n", _fields(I, I))[2] == 0 and decode(b"only,header", _fields(I, I))[2] == 0
    cols, _, rows = decode(b"7", _fields(I), has_header=False)
    assert rows == 1 and cols["c0"].tolist() == [7]


def test_trailing_delimiter_column_and_other_delimiters():
    cols, _, rows = decode(b"1|ab|2.5|\n2|c,d|-1e3|\n", _fields(L, S, D, None), delimiter=b"|", has_header=False)
    assert rows == 2 and cols["c0"].tolist() == [1, 2] and _strings(cols["c1"]) == [b"ab", b"c,d"] and cols["c2"].tolist() == [2.5, -1000.0]
    assert "c3" not in cols
    cols, _, rows = decode(b"1\t\"a\tb\"\n", _fields(U, S), delimiter=b"\t", has_header=False)
    assert rows == 1 and cols["c0"].tolist() == [1] and _strings(cols["c1"]) == [b"a\tb"]
    with pytest.raises(CsvError) as e:       # without the SKIP column the trailing '|' is one field too many
        decode(b"1|ab|2.5|\n", _fields(L, S, D), delimiter=b"|", has_header=False)
    assert (e.value.status, e.value.record, e.value.code) == ("invalid", 1, "many_fields")


def test_nulls():
    text = b'i,l,u,d,t,s\n,,,,,\n"","","","","",""\n1,2,3,4.5,2020-01-02,x\n'
    cols, valid, rows = decode(text, _fields(I, L, U, D, T, S))
    assert rows == 3
    for k in range(5):
        assert valid["c%d" % k].tolist() == [0, 0, 1] and cols["c%d" % k][:2].tolist() == [0, 0]
    assert "c5" not in valid and _strings(cols["c5"]) == [b"", b"", b"x"]
    assert cols["c4"][2] == 1577923200000 and cols["c3"][2] == 4.5 and cols["c2"].dtype == np.uint64


def test_values():
    cols, _, _ = decode(b'+5,-0,18446744073709551615,"2020-11-01 00:11:32.6250",0000000000000000000000000000012\n', _fields(I, L, U, T, I), has_header=False)
    assert cols["c0"].tolist() == [5] and cols["c1"].tolist() == [0] and cols["c2"].tolist() == [2**64 - 1] and cols["c4"].tolist() == [12]
    assert cols["c3"].tolist() == [parse_timestamp("2020-11-01 00:11:32.625")] == [1604189492625]
    assert parse_timestamp("2020-11-01 00:11:32.123456789") == 1604189492123 and parse_timestamp("2020-11-01 00:11:32.1234567890") is None
    assert parse_timestamp("2020-11-01 00:11:32.12x4") is None and parse_timestamp("2020-11-01 00:11:3.21234") is None


ERRORS = [
    # text, fields, (status, record, column, code); the header is record 1
    (b"a,b\n1,2\n\n3,4\n", (I, I), ("unsupported", 3, 0, "blank")),
    (b"a,b\n1,2\n\r\n3,4\n", (I, I), ("unsupported", 3, 0, "blank")),
    (b"a,b\n1,2\n3,x\ry\n", (I, S), ("unsupported", 3, 1, "bare_cr")),
    (b"a,b\n1,2\r", (I, I), ("unsupported", 2, 1, "bare_cr")),
    (b'a,b\n1,2\n3,x"y\n', (I, S), ("invalid", 3, 1, "stray_quote")),
    (b'a,b\n1,"x"y\n3,4\n', (I, S), ("invalid", 2, 1, "after_quote")),
    (b'a,b\n1,"x" \n', (I, S), ("invalid", 2, 1, "after_quote")),
    (b'a,b\n1,2\n3,"never closed\n5,6\n', (I, S), ("invalid", 3, 1, "open_quote")),
    (b'a,b\n1,"ends in a doubled quote""', (I, S), ("invalid", 2, 1, "open_quote")),
    (b"a,b,c\n1,2,3\n4,5\n", (I, I, I), ("invalid", 3, 1, "few_fields")),
    (b"a,b\n1,2\n3,4,5\n", (I, I), ("invalid", 3, 1, "many_fields")),
    (b"a,b\n1,2147483648\n", (I, I), ("invalid", 2, 1, "value")),
    (b"a,b\n1,-2147483648\n2,1.5\n", (I, I), ("invalid", 3, 1, "value")),
    (b"a\n-1\n", (U,), ("invalid", 2, 0, "value")),
    (b"a\n2020-02-30\n", (T,), ("invalid", 2, 0, "value")),
    (b"a\n1.0\n0.1234567890123456789\n", (D,), ("unsupported", 3, 0, "float")),
    (b"a\n1e23\n", (D,), ("unsupported", 2, 0, "float")),
    (b"a\nnan\n", (D,), ("unsupported", 2, 0, "float")),
    (b"a\n0x10\n", (D,), ("unsupported", 2, 0, "float")),
    (b"a,b\nx,2\n3,\"\n", (I, I), ("invalid", 2, 0, "value")),       # the first failure in stream order, not the worst
    (b'a,b\n1,"2""3"\n', (I, I), ("invalid", 2, 1, "value")),          # a quoted number that holds '""'
]


@pytest.mark.parametrize("case", range(len(ERRORS)))
def test_errors(case):
    text, types, want = ERRORS[case]
    with pytest.raises(CsvError) as e:
        decode(text, _fields(*types))
    assert (e.value.status, e.value.record, e.value.column, e.value.code) == want


# ---- the seeded corpus against csv.reader and pyarrow ---------------------------------------------------------------------------------------------------------------
_ALPHABET = ["a", "b", "Z", " ", "0", "9", "-", ".", ",", "|", "\t", '"', "\n", "\r\n", "\r", "é", "漢", "'", ";"]


def _value(r, ty):
    if ty == S:
        return "".join(r.choice(_ALPHABET) for _ in range(r.choice((0, 1, 3, 8, 30))))
    if r.random() < 0.1:
        return ""                                    # NULL
    if ty == I:
        return str(r.choice((0, 1, -1, 2**31 - 1, -2**31, r.randrange(-2**31, 2**31))))
    if ty == L:
        return "0" * r.choice((0, 0, 3)) + str(r.choice((2**63 - 1, r.randrange(0, 2**63)))) if r.random() < 0.5 else str(r.randrange(-2**63, 0))
    if ty == U:
        return str(r.choice((0, 2**64 - 1, r.randrange(0, 2**64))))
    if ty == D:
        return _float_text(r)
    d = "%04d-%02d-%02d" % (r.randrange(1, 10000), r.randrange(1, 13), r.randrange(1, 29))
    k = r.randrange(3)
    return d if k == 0 else d + " %02d:%02d:%02d" % (r.randrange(24), r.randrange(60), r.randrange(60)) + ("" if k == 1 else ".%03d" % r.randrange(1000))


def _float_text(r):
    """A decimal text inside A-CSV5's exact range: at most 2^53 as significand, exponent after folding in [-22, 22]."""
    w = r.choice((0, 1, 2**53, r.randrange(0, 2**53 + 1), r.randrange(0, 10**6)))
    w += 1 if w and w % 10 == 0 else 0               # (zeros at the significand's end move the exponent: k == 4 writes them on purpose)
    digits = str(w)
    sign = r.choice(("", "-"))
    k = r.randrange(5)
    if k == 0:
        return sign + digits
    if k == 4:
        z = r.randrange(1, 23)
        return sign + digits + "0" * z + "e" + str(r.randrange(-22 - z, 23 - z))
    if k == 1:                                       # a point inside, or zeros in front of the digits behind the point
        cut = r.randrange(0, min(len(digits), 22) + 1)
        return sign + (digits[:len(digits) - cut] or "0") + "." + (digits[len(digits) - cut:] or "0")
    e = r.randrange(-22, 23)
    if k == 2:
        return sign + digits + r.choice("eE") + ("+" if e >= 0 and r.random() < 0.5 else "") + str(e)
    cut = r.randrange(0, len(digits) + 1)            # a point and an exponent: the folded exponent is e - cut
    e = max(e, -22 + cut)
    return sign + (digits[:len(digits) - cut] or "0") + "." + (digits[len(digits) - cut:] or "0") + "e" + str(e)


def _write(r, rows, delim, eol, final_eol):
    """Our own writer: quotes what must be quoted (delimiter, quote, CR, LF inside; a Utf8 value that would read as something else) and some of the rest."""
    out = []
    for row in rows:
        cells = []
        for v, ty in row:
            must = any(c in v for c in (delim, '"', "\n", "\r"))
            if must or (v != "" and r.random() < 0.2) or (ty == S and v == "" and r.random() < 0.5):
                v = '"' + v.replace('"', '""') + '"'
            cells.append(v)
        out.append(delim.join(cells))
    return (eol.join(out) + (eol if final_eol else "")).encode("utf-8")


def corpus(seed, n_rows=120):
    r = random.Random(seed)
    types = [r.choice((I, L, U, D, T, S, S)) for _ in range(r.randrange(2, 9))]      # (at least two columns: a row of one empty field is a blank line)
    types[0] = S
    delim = r.choice((",", "|", "\t"))
    rows = [[(_value(r, t), t) for t in types] for _ in range(n_rows)]
    header = [("h%d" % i, S) for i in range(len(types))]
    return _write(r, [header] + rows, delim, r.choice(("\n", "\r\n")), r.random() < 0.7), delim, types, rows


@pytest.mark.parametrize("seed", range(12))
def test_corpus_against_csv_module_and_pyarrow(seed):
    pa = pytest.importorskip("pyarrow")
    import pyarrow.csv as pacsv
    text, delim, types, rows = corpus(seed)
    fields = _fields(*types)
    cols, valid, n = decode(text, fields, delimiter=delim.encode())
    assert n == len(rows)
    # the field split, against csv.reader(strict=True) (newline='' hands it the terminators as they are)
    want = list(csv.reader(io.StringIO(text.decode("utf-8"), newline=""), delimiter=delim, strict=True))[1:]
    got = [[f.decode("utf-8") for f in rec] for _, rec in csv_ref.records(text, delim.encode())][1:]
    assert got == want == [[v for v, _ in row] for row in rows]
    # the typed columns, against pyarrow
    pa_types = {I: pa.int32(), L: pa.int64(), U: pa.uint64(), D: pa.float64(), T: pa.timestamp("ms"), S: pa.string()}
    table = pacsv.read_csv(io.BytesIO(text), parse_options=pacsv.ParseOptions(delimiter=delim, newlines_in_values=True),
                           read_options=pacsv.ReadOptions(column_names=[name for name, _ in fields], skip_rows=1),
                           convert_options=pacsv.ConvertOptions(null_values=[""], strings_can_be_null=False,
                                                                column_types={name: pa_types[t] for name, t in fields}))
    assert table.num_rows == n
    for name, t in fields:
        col = table[name].combine_chunks()
        if t == S:
            assert [s.encode("utf-8") for s in col.to_pylist()] == _strings(cols[name]) and col.null_count == 0
            continue
        assert np.array_equal(np.array(col.is_valid().to_pylist(), dtype=np.uint8), valid[name]), name
        ref = col.cast(pa.int64()) if t == T else col
        for i, v in enumerate(ref.to_pylist()):
            if v is not None:
                if t == D:
                    assert struct.pack("<d", v) == struct.pack("<d", float(cols[name][i])), (name, i)
                else:
                    assert v == int(cols[name][i]), (name, i)


# ---- Float64 against float(), both directions -------------------------------------------------------------------------------------------------------------------
def test_float_accepts_only_exact_and_refuses_nothing_inside_the_range():
    r = random.Random(53)
    texts = [_float_text(r) for _ in range(20000)]
    for s in texts:                                                  # inside the exact range nothing is refused ...
        v = parse_float(s)
        assert v is not None, s
    # ... and whatever is accepted, of ANY text, is float()'s double bit for bit (the sign of zero included)
    digits = "0123456789"
    for _ in range(20000):
        k = r.randrange(1, 26)
        s = r.choice(("", "-", "+")) + "".join(r.choice(digits) for _ in range(k))
        if r.random() < 0.6:
            p = r.randrange(0, len(s) + 1)
            s = s[:p] + "." + s[p:]
        if r.random() < 0.5:
            s += r.choice("eE") + r.choice(("", "-", "+")) + str(r.randrange(0, 40))
        texts.append(s)
    texts += ["9007199254740992", "9007199254740993", "9007199254740992e22", "9007199254740992e23", "1e22", "1e23", "1e-22", "1e-23", "0e999", "-0", "-0.000e-999",
              "8.5", "123456789012345678", "1234567890123450000000", "0.3", "3e-1", "1.", ".5", "", "e5", "1e", "1e+", "inf", "nan", "0x1p3", "1_0", " 1", "1 ",
              "179769313486231570000000000000000000000e270", "4.9e-324", "100000000000000000000000"]
    accepted = 0
    for s in texts:
        v = parse_float(s)
        if v is not None:
            accepted += 1
            assert struct.pack("<d", v) == struct.pack("<d", float(s)), s
    assert accepted > 25000
    for s in ("9007199254740993", "1e23", "1e-23", "9007199254740992e23", "1.", ".5", "", "inf", "nan", "0x1p3", "1_0", " 1", "123456789012345678", "4.9e-324"):
        assert parse_float(s) is None, s
    for s, bits in (("9007199254740992", 2.0**53), ("1e22", 1e22), ("1234567890123450000000", 1.23456789012345e21), ("0e999", 0.0)):
        assert parse_float(s) == bits, s
    assert struct.pack("<d", parse_float("-0")) == struct.pack("<d", -0.0)


# ---- the fixtures: not one field refused ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(csv_ref.FIXTURES))
def test_fixture_decodes_with_no_field_refused(name):
    text, delim, header, fields = csv_ref.fixture(name)
    as_text, _, rows = decode(text, [(n, None if t is None else S) for n, t in fields], delimiter=delim, has_header=header)
    assert rows == {"citibike": 214}.get(name, rows) and rows > 0
    refused = 0
    for n, t in fields:
        if t not in (None, S):
            refused += sum(1 for raw in _strings(as_text[n]) if raw != b"" and csv_ref.parse_value(raw, t) is None)
    assert refused == 0
    cols, valid, rows2 = decode(text, fields, delimiter=delim, has_header=header)
    assert rows2 == rows and set(cols) == {n for n, t in fields if t is not None}
    if name == "citibike":      # quoted timestamps with four fraction digits; 15 columns
        assert cols["starttime"][0] == 1604189492625 and cols["start_station_latitude"][0] == 40.71835519823214 and len(fields) == 15
    if name == "uk_cities":     # quoted commas
        assert _strings(cols["city"])[0] == b"Elgin, Scotland, the UK" and cols["lat"][0] == 57.653484 and cols["lng"][0] == -3.335724
    if name == "lineitem0":     # dates as Timestamp(ms) and as Utf8
        assert cols["l_shipdate"][0] == 826675200000 and _strings(cols["l_receiptdate"])[0] == b"1996-03-22"


# ---- csv.hpp itself, on the host under ASan / UBSan ---------------------------------------------------------------------------------------------------------------------
def test_csv_hpp_host_program():
    exe = os.path.join(ROOT, "tests", "cpp", "csv_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "flock_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "csv_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "csv_test: ok" in out.stdout, out.stdout + out.stderr
