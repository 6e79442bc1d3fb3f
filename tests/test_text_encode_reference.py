"""tests/text_encode_ref.py -- the reference of textenc.hpp's A-ENC1..10 that the GPU tests compare bytes against -- checked against independent
implementations on the CPU: json.dumps / json.loads row by row, oracle.nexmark_json_lines on generated events, csv_ref.decode (the CSV decoder's
reference) as the round trip, and csv.reader(strict=True) on the text columns (on a corpus without NUL, which this Python's csv module refuses).
textenc.hpp itself runs as a stand-alone host program (tests/cpp/textenc_test.cpp)."""
import csv
import io
import json
import os
import random
import subprocess

import numpy as np
import pytest

import csv_ref
import oracle
import text_encode_ref as ref
from test_oracle_json import SCHEMAS, _events

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, L, U, T, S = "int32", "int64", "uint64", "timestamp_ms", "utf8"
ALPHABET = [",", "|", '"', "\n", "\r", "\\", "\t", "\0", "\x08", "\x0c", "\x1f", "\x7f", "/", "é", "\U0001F600"] + list("abcxyz 09")
EXTREMES = {I: [-2**31, 2**31 - 1, 0, -1], L: [-2**63, 2**63 - 1, 0, -1], U: [2**64 - 1, 2**63, 0, 1],
            T: [ref.TS_MIN, ref.TS_MAX, -1, 999, 1000, 0]}
WEIRD = 'we"ird,name'


def _value(r, t, alphabet, long_ok):
    if t == S:
        n = 5000 if long_ok and r.random() < 0.01 else r.randrange(0, 41)
        common = r.random() < 0.5        # half of the values hold no class byte
        return "".join(r.choice("abcxyz 09/" if common else alphabet) for _ in range(n)).encode()
    if r.random() < 0.15:
        return r.choice(EXTREMES[t])
    if t == T:
        return r.randrange(ref.TS_MIN, ref.TS_MAX + 1) if r.random() < 0.5 else 1_436_918_400_000 + r.randrange(-10**9, 10**9) * r.choice((1, 1000))
    bits = r.choice((8, 16, 31, 62))
    return r.randrange(0, 2**bits) if t == U else r.randrange(-2**bits, 2**bits) if t != I else r.randrange(-2**min(bits, 31), 2**min(bits, 31))


def corpus(seed, n_rows=400, types=None, nul=True, nulls=True, long_ok=True):
    """(columns, valid) for the encoders: every type at least once, the alphabet of class bytes, the type extremes, NULLs in every type."""
    r = random.Random(seed)
    types = list(types) if types else [S, I, L, U, T, S] + [r.choice((I, L, U, T, S)) for _ in range(r.randrange(0, 4))]
    alphabet = [c for c in ALPHABET if nul or c != "\0"]
    names = ["c%d" % i for i in range(len(types))]
    if len(types) > 1:
        names[1] = WEIRD
    columns, valid = [], {}
    for name, t in zip(names, types):
        vals = [_value(r, t, alphabet, long_ok) for _ in range(n_rows)]
        if t == S:
            col = ref.utf8_of(vals)
        elif t == U:
            col = np.array(vals, np.uint64).view(np.int64)        # (the bits, as the device takes them)
        else:
            col = np.array(vals, np.int32 if t == I else np.int64)
        columns.append((name, t, col))
        if nulls and r.random() < 0.8:
            valid[name] = np.array([r.random() >= 0.2 for _ in range(n_rows)], np.uint8)
    return columns, valid


def as_fields(columns):
    return [(name, t) for name, t, _ in columns]


def _python_rows(columns, valid):
    """Per row the {name: value} dict json.dumps takes (None = NULL)."""
    cells = []
    for name, t, col in columns:
        vals = [s.decode("utf-8") for s in ref.strings_of(col)] if t == S else [int(v) % 2**64 if t == U else int(v) for v in col]
        ok = valid.get(name)
        cells.append([v if ok is None or ok[i] else None for i, v in enumerate(vals)])
    return [{name: cells[c][i] for c, (name, _, _) in enumerate(columns)} for i in range(len(cells[0]))]


# ---- JSON ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_json_agrees_with_json_dumps(seed):
    columns, valid = corpus(seed)
    text = ref.json_lines(columns, valid)
    lines = text.split(b"\n")
    assert lines.pop() == b"" and len(lines) == 400        # every row newline-terminated, and an escaped '\n' never ends a line
    rows = _python_rows(columns, valid)
    for line, row in zip(lines, rows):
        assert line == json.dumps(row, separators=(",", ":"), ensure_ascii=False).encode("utf-8")
        assert json.loads(line) == row
    assert ref.json_lines([(n, t, c[:0] if t != S else ref.utf8_of([])) for n, t, c in columns]) == b""


@pytest.mark.parametrize("relation", ["bid", "auction", "person"])
def test_json_agrees_with_the_generator_oracle(relation):
    cols = _events(relation)
    columns = [(name, t, cols[name]) for name, t in SCHEMAS[relation]]
    assert ref.json_lines(columns) == oracle.nexmark_json_lines(relation, cols)


# ---- CSV -----------------------------------------------------------------------------------------------------------------------------------------------------
def _same_columns(got, got_valid, n, columns, valid):
    assert n == (len(columns[0][2].offsets) - 1 if columns[0][1] == S else len(columns[0][2]))
    for name, t, col in columns:
        ok = valid.get(name, np.ones(n, np.uint8))
        if t == S:      # a NULL Utf8 comes back as ''
            want = [s if ok[i] else b"" for i, s in enumerate(ref.strings_of(col))]
            assert ref.strings_of(got[name]) == want, name
            continue
        assert np.array_equal(got_valid[name], ok), name
        assert np.array_equal(got[name].view(np.int64 if t != I else np.int32)[ok != 0], col[ok != 0]), name


@pytest.mark.parametrize("header", [True, False])
@pytest.mark.parametrize("delim", [b",", b"|"])
@pytest.mark.parametrize("seed", range(3))
def test_csv_round_trip_through_the_decoder_reference(seed, delim, header):
    columns, valid = corpus(seed)
    text = ref.csv_text(columns, valid, delimiter=delim, has_header=header)
    got, got_valid, n = csv_ref.decode(text, as_fields(columns), delimiter=delim, has_header=header)
    _same_columns(got, got_valid, n, columns, valid)


@pytest.mark.parametrize("delim", [",", "|"])
@pytest.mark.parametrize("seed", range(3))
def test_csv_agrees_with_the_csv_module(seed, delim):
    columns, valid = corpus(seed, nul=False)
    text = ref.csv_text(columns, valid, delimiter=delim.encode(), has_header=True)
    records = list(csv.reader(io.StringIO(text.decode("utf-8"), newline=""), delimiter=delim, strict=True))
    assert records[0] == [name for name, _, _ in columns] and len(records) == 401
    for c, (name, t, col) in enumerate(columns):
        if t != S:
            continue
        ok = valid.get(name, np.ones(400, np.uint8))
        assert [rec[c] for rec in records[1:]] == [s.decode("utf-8") if ok[i] else "" for i, s in enumerate(ref.strings_of(col))], name


def test_one_column_tables_have_no_blank_line():
    for t, col in ((S, ref.utf8_of([b"a", b"", b"b"])), (I, np.array([1, 2, 3], np.int32)), (T, np.array([0, 1, 1000], np.int64))):
        text = ref.csv_text([("c", t, col)], {"c": np.array([1, 0, 1], np.uint8)}, has_header=False)
        assert text.split(b"\n")[1] == b'""' and b"\n\n" not in text
        got, got_valid, n = csv_ref.decode(text, [("c", t)], has_header=False)
        assert n == 3 and (t == S or got_valid["c"].tolist() == [1, 0, 1])
    assert ref.csv_text([("c", S, ref.utf8_of([b"", b"x"]))], has_header=False) == b'""\nx\n'        # '' and NULL both come out as ""


def test_refusals_of_the_reference():
    col = np.zeros(3, np.int64)
    for columns, status in (([], "invalid"), ([("c%d" % i, L, col) for i in range(65)], "unsupported"), ([("x" * 32, L, col)], "unsupported"),
                            ([("", L, col)], "unsupported"), ([("c", "float64", col.view(np.float64))], "unsupported")):
        with pytest.raises(ref.EncodeError) as e:
            ref.json_lines(columns)
        assert e.value.status == status
    with pytest.raises(ref.EncodeError) as e:
        ref.csv_text([("c", L, col)], delimiter=b'"')
    assert e.value.status == "invalid"
    ts = np.zeros(1000, np.int64)
    ts[699], ts[299] = ref.TS_MAX + 1, ref.TS_MIN - 1
    with pytest.raises(ref.EncodeError) as e:
        ref.csv_text([("a", L, ts), ("t", T, ts)])
    assert (e.value.status, e.value.record, e.value.column) == ("invalid", 301, 1)
    assert ref.json_lines([("t", T, ts[298:300])]) == b'{"t":0}\n{"t":%d}\n' % (ref.TS_MIN - 1)


def test_timestamp_text():
    for ms, want in ((0, b"1970-01-01 00:00:00"), (-1, b"1969-12-31 23:59:59.999"), (999, b"1970-01-01 00:00:00.999"), (1000, b"1970-01-01 00:00:01"),
                     (ref.TS_MIN, b"0000-01-01 00:00:00"), (ref.TS_MAX, b"9999-12-31 23:59:59.999"), (1456704000000, b"2016-02-29 00:00:00"),
                     (951782400000, b"2000-02-29 00:00:00"), (-2203891200000, b"1900-03-01 00:00:00")):
        assert ref.timestamp_text(ms) == want
        assert csv_ref.parse_timestamp(want.decode()) == ms


# ---- textenc.hpp itself, on the host -----------------------------------------------------------------------------------------------------------------------------
def test_textenc_hpp_host_program():
    exe = os.path.join(ROOT, "tests", "cpp", "textenc_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "flock_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "textenc_test.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "textenc_test: ok" in out.stdout, out.stdout + out.stderr


def test_both_entry_points_are_bound():
    from flock_amd import _ffi
    assert "flockgpu_json_lines_encode" in _ffi.SYMBOLS and "flockgpu_csv_encode" in _ffi.SYMBOLS
