"""Delimited text -> columns on the GPU (flockgpu_csv_decode, csv.hip) against tests/csv_ref.py, the reference of csv.hpp's A-CSV1..7 (itself checked against
csv.reader and pyarrow in tests/test_csv_reference.py).  Every comparison is exact: values, validity, offsets, bytes.  The fixtures with their real schemas,
a generated bid relation as CSV, quote state across the 16 KiB tiles of the record index, records that leave the LDS stage, edge inputs, NULLs, every
error, the text at the end of a mapping, and q13 fed from a CSV side input."""
import os
import sys

import numpy as np
import pytest

import csv_ref
import oracle
from test_csv_reference import ERRORS, corpus
from test_oracle_json import _events

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 16384          # bytes per tile of the record index (csv.hip kIdxTile)
I, L, U, D, T, S = "int32", "int64", "uint64", "float64", "timestamp_ms", "utf8"
TYPE_NAMES = csv_ref.TYPE_NAMES


@pytest.fixture(scope="module")
def ctx():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def _dev_bytes(b, at_end=False):
    """The text on the device, 16-byte aligned.  at_end: it ENDS where the allocation's 16-byte granule ends when its length allows (and where mapped
    memory ends under FLOCK_TEST_GUARDED=1, tests/test_gpu_guard.py), so that a 16-byte load over the last partial chunk leaves the buffer."""
    from devmem import dev, guarded
    if guarded():
        return dev(np.frombuffer(bytes(b), np.uint8))
    import torch
    t = torch.zeros((len(b) + 15) // 16 * 16 + (0 if at_end else 16), dtype=torch.uint8, device="cuda")
    if len(b):
        t[: len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    return t[: len(b)]


def _fields(*types):
    return [("c%d" % i, t) for i, t in enumerate(types)]


def _same(got, valid, n, want, want_valid, want_n, fields):
    assert n == want_n
    for name, t in fields:
        if t is None:
            assert name not in got
            continue
        if t == S:
            off = got[name].offsets.cpu().numpy()
            assert np.array_equal(off, want[name].offsets), name
            assert np.array_equal(got[name].data.cpu().numpy()[: off[-1]], want[name].data), name
            assert name not in valid
            continue
        g = got[name].cpu().numpy()
        assert g.dtype == (np.int64 if t == U else want[name].dtype) and len(g) == n
        assert np.array_equal(g.view(np.uint8), want[name].view(np.uint8)), name          # bit for bit: Float64 and the sign of zero included
        if want_valid[name].all():
            assert name not in valid, name                                                 # no NULL: no validity in the Python result
        else:
            assert np.array_equal(valid[name].cpu().numpy(), want_valid[name]), name


def _check(ctx, text, fields, delimiter=b",", has_header=True, **kw):
    want, want_valid, want_n = csv_ref.decode(text, fields, delimiter=delimiter, has_header=has_header)
    got, valid, n = ctx.csv_decode(_dev_bytes(text), fields, delimiter=delimiter, has_header=has_header, **kw)
    _same(got, valid, n, want, want_valid, want_n, fields)
    return got, valid, n


# ---- the fixtures with their real schemas ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(csv_ref.FIXTURES))
def test_fixtures(ctx, name):
    text, delim, header, fields = csv_ref.fixture(name)
    _, _, n = _check(ctx, text, fields, delim, header)
    assert n > 0


@pytest.mark.parametrize("seed", range(4))
def test_seeded_corpus(ctx, seed):
    text, delim, types, rows = corpus(seed, n_rows=700)
    _, _, n = _check(ctx, text, _fields(*types), delim.encode())
    assert n == 700


# ---- a generated bid relation ------------------------------------------------------------------------------------------------------------------------------------------
BID = [("auction", I), ("bidder", I), ("price", I), ("b_date_time", L)]


@pytest.mark.parametrize("n_events", [4000, 300_000])
def test_generated_bids(ctx, n_events):
    cols = _events("bid", n_events)
    n = len(cols["auction"])
    assert n > 0
    text = ("auction,bidder,price,b_date_time\n" + "".join("%d,%d,%d,%d\n" % r for r in zip(*(cols[k].tolist() for k, _ in BID)))).encode()
    assert n_events < 300_000 or (n > 256 and len(text) > 4 * TILE)          # more than one workgroup, several index tiles
    for t, kw in ((text, {}), (text[:-1], {}), (text, {"borrow": True})):    # with and without the final newline; the library's own columns in place
        got, valid, rows = ctx.csv_decode(_dev_bytes(t), BID, **kw)
        assert rows == n and valid == {}
        for k, _ in BID:
            assert np.array_equal(got[k].cpu().numpy(), cols[k]), k
    if n_events == 4000:
        _check(ctx, text, BID)


# ---- quote state across the tiles of the index ----------------------------------------------------------------------------------------------------------------------------
def _fill(n):
    """n bytes of short well-formed (Int32, Utf8) records, n >= 4."""
    out = b"7,xxxxx\n" * ((n - 8) // 8 if n >= 16 else 0)
    rest = n - len(out)
    return out + b"7," + b"y" * (rest - 3) + b"\n"


def _at(record, key, where):
    """A text in which byte `key` of `record` lies at offset `where`, with records before and after it."""
    text = b"k,s\n" + _fill(where - key - 4) + record + b"8,after\n" * 3
    assert text[where] == record[key]
    return text


def test_quoted_field_over_three_tiles(ctx):
    big = (b"line, with a delimiter\n" * 2300)[: 50_000]
    text = b"k,s\n1,before\n2,\"" + big + b"\"\n3,after\n"
    assert len(text) > 3 * TILE
    got, _, n = _check(ctx, text, _fields(I, S))
    assert n == 3 and got["c0"].cpu().tolist() == [1, 2, 3]


@pytest.mark.parametrize("where", [TILE - 1, TILE, 2 * TILE - 1, 2 * TILE])
def test_closing_quote_at_a_tile_seam(ctx, where):
    rec = b'5,"a,b\nc"\n'          # the closing quote: last byte of a tile, first byte of the next
    _, _, n = _check(ctx, _at(rec, rec.index(b'"\n'), where), _fields(I, S))
    assert n > 100


def test_doubled_quote_and_crlf_split_across_a_seam(ctx):
    rec = b'5,"a""b,\n"\n'
    got, _, _ = _check(ctx, _at(rec, rec.index(b'""') + 1, TILE), _fields(I, S))          # '"' | '"'
    rec = b"5,tail\r\n"
    _check(ctx, _at(rec, rec.index(b"\n"), TILE), _fields(I, S))                           # '\r' | '\n'
    rec = b'5,"tail"\r\n'
    _check(ctx, _at(rec, rec.index(b"\n"), 2 * TILE), _fields(I, S))
    rec = b'5,"open\n'                                                                     # the opening quote first in a tile, a newline right behind it
    _check(ctx, _at(rec + b'still,"" inside"\n', rec.index(b'"'), TILE), _fields(I, S))


def test_alternating_quoted_and_unquoted(ctx):
    lines = [b"a,b,c,d"]
    for i in range(10_000):
        q = [(b'"%d"' if (i + k) % 2 else b"%d") % (i * 4 + k) for k in range(3)]
        lines.append(b",".join(q) + (b',"t,%d\n""x"""' % i if i % 2 else b",plain%d" % i))
    text = b"\n".join(lines) + b"\n"
    got, _, n = _check(ctx, text, _fields(I, L, U, S))
    assert n == 10_000


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_record_longer_than_the_lds_stage(ctx):
    long = b"z" * 70_000
    text = b"s,i,d,t\n" + b"".join(b"r%d,%d,%d.5,2021-03-04 05:06:07\n" % (i, i, i) for i in range(300)) + \
        long + b",-123,4.25,2020-11-01 00:11:32.6250\n" + b'"' + long[:60_000] + b'""",77,1e22,\nlast,1,2,1999-12-31\n'
    got, valid, n = _check(ctx, text, _fields(S, I, D, T))
    assert n == 303 and got["c1"].cpu().tolist()[300:302] == [-123, 77] and valid["c3"].cpu().tolist()[301] == 0
    _check(ctx, long + b"|5|\n", _fields(S, I, None), delimiter=b"|", has_header=False)      # one record, all of it past the stage


def test_numeric_field_longer_than_a_window(ctx):
    text = b"a,b,c\n" + b"0" * 40 + b"12,-" + b"0" * 30 + b"9223372036854775808,+" + b"0" * 25 + b"18446744073709551615\n1,2,3\n"
    got, _, _ = _check(ctx, text, _fields(I, L, U))
    assert got["c0"].cpu().tolist() == [12, 1] and got["c1"].cpu().tolist() == [-2**63, 2]


# ---- edge inputs --------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_edge_inputs(ctx):
    for header in (True, False):
        got, valid, n = _check(ctx, b"", _fields(I, S, D), has_header=header)
        assert n == 0 and len(got["c0"]) == 0 and got["c1"].offsets.cpu().tolist() == [0]
    _check(ctx, b"just,a,header\n", _fields(I, S, D))
    _check(ctx, b"just,a,header", _fields(I, S, D))
    got, _, n = _check(ctx, b"1,x,2.5", _fields(I, S, D), has_header=False)                  # one record without terminator
    assert n == 1 and got["c2"].cpu().tolist() == [2.5]
    got, _, n = _check(ctx, b"h\n5\n\"6\"\n7", _fields(I))                                    # n_fields = 1
    assert got["c0"].cpu().tolist() == [5, 6, 7]
    _check(ctx, b"x", _fields(S), has_header=False)
    _check(ctx, b"\"\"\n", _fields(S), has_header=False)                                      # ONE empty quoted field is no blank line


def test_64_columns_and_skips(ctx):
    types = [(I, L, U, D, T, S, None, S)[k % 8] for k in range(64)]
    cell = {I: b"-%d", L: b"%d000000000", U: b"1%d", D: b"%d.25", T: b"2001-02-03 04:05:%02d", S: b'"s,%d"', None: b"skipped%d"}
    text = b"\n".join(b",".join(cell[t] % ((r + k) % 60) for k, t in enumerate(types)) for r in range(600)) + b"\n"
    _check(ctx, text, _fields(*types), has_header=False)
    only = [None] * 64
    only[41] = L
    got, _, n = _check(ctx, text, _fields(*only), has_header=False)                            # all columns SKIP but one
    assert n == 600 and list(got) == ["c41"]
    from flock_amd import FlockGpuError, _ffi
    with pytest.raises(FlockGpuError) as e:
        ctx.csv_decode(_dev_bytes(b"1\n"), _fields(*([I] * 65)), has_header=False)
    assert e.value.code == _ffi.ERR_UNSUPPORTED


# ---- NULLs -----------------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_nulls(ctx):
    text = b'i,l,u,d,t,s\n,,,,,\n"","","","","",""\n1,2,3,4.5,2020-01-02,x\n' + b"9,8,7,-0,1970-01-01,\n" * 500 + b',1,,2,,""\n'
    got, valid, n = _check(ctx, text, _fields(I, L, U, D, T, S))
    assert n == 504 and sorted(valid) == ["c0", "c1", "c2", "c3", "c4"]
    assert [int((valid[k].cpu().numpy() == 0).sum()) for k in sorted(valid)] == [3, 2, 3, 2, 3]         # null_count is what brings validity along
    assert got["c0"].cpu().tolist()[:3] == [0, 0, 1] and got["c5"].offsets.cpu().tolist()[:4] == [0, 0, 0, 1]
    got, valid, _ = _check(ctx, b"a,b\n1,\n2,x\n", _fields(I, S))
    assert valid == {}                                                                                  # an empty Utf8 is '', never NULL
    # the C ABI's null_count, and validity written even where no row is NULL
    import ctypes as C
    from flock_amd import _ffi
    t = _dev_bytes(b"a,b\n1,\n,x\n3,\n")
    spec = (_ffi.CsvField * 2)(_ffi.CsvField(_ffi.CSV_INT64), _ffi.CsvField(_ffi.CSV_UTF8))
    opt, cols, rows = _ffi.CsvOptions(ord(","), 1), (_ffi.CsvColumn * 2)(), C.c_int64(0)
    assert ctx._lib.flockgpu_csv_decode(ctx._h, t.data_ptr(), t.numel(), spec, 2, C.byref(opt), cols, C.byref(rows)) == _ffi.OK
    assert rows.value == 3 and cols[0].null_count == 1 and cols[1].null_count == 0 and cols[0].valid and not cols[1].valid
    assert ctx.d2h(cols[0].valid, 3, np.uint8).tolist() == [1, 0, 1] and ctx.d2h(cols[0].values, 3, np.int64).tolist() == [1, 0, 3]


# ---- errors ------------------------------------------------------------------------------------------------------------------------------------------------------------------------
MESSAGES = {"blank": "blank line", "bare_cr": "bare CR", "stray_quote": "quote inside an unquoted field", "after_quote": "closing quote",
            "open_quote": "unterminated quote", "few_fields": "fields where", "many_fields": "more than the", "value": "does not parse as", "float": "Float64"}


@pytest.mark.parametrize("case", range(len(ERRORS)))
def test_errors(ctx, case):
    from flock_amd import FlockGpuError, _ffi
    text, types, (status, record, column, code) = ERRORS[case]
    fields = _fields(*types)
    with pytest.raises(csv_ref.CsvError):
        csv_ref.decode(text, fields)
    with pytest.raises(FlockGpuError) as e:
        ctx.csv_decode(_dev_bytes(text), fields)
    msg = str(e.value)
    assert e.value.code == (_ffi.ERR_UNSUPPORTED if status == "unsupported" else _ffi.ERR_INVALID), msg
    assert "record %d:" % record in msg and MESSAGES[code] in msg, msg
    if code not in ("blank", "few_fields", "many_fields"):
        assert "column %d:" % column in msg, msg
    if code == "value":
        assert msg.endswith("as " + TYPE_NAMES[types[column]]), msg
    _check(ctx, b"a,b\n1,x\n2,\"y\"\n", _fields(I, S))                      # afterwards the context decodes a good text


def test_first_offender_among_many_records(ctx):
    """The record number over many workgroups and index tiles: the FIRST bad record wins, whichever lane finds one first."""
    from flock_amd import FlockGpuError, _ffi
    lines = [b"k,v"] + [b"%d,%d.5" % (i, i) for i in range(40_000)]
    bad = {39_000: (b"1,1e400", _ffi.ERR_UNSUPPORTED), 20_001: (b"2147483648,1", _ffi.ERR_INVALID), 777: (b"7", _ffi.ERR_INVALID)}
    for at, (line, _) in bad.items():
        lines[at] = line
    text = b"\n".join(lines) + b"\n"
    for record in (777, 20_001, 39_000):
        with pytest.raises(FlockGpuError) as e:
            ctx.csv_decode(_dev_bytes(text), _fields(I, D))
        assert "record %d:" % (record + 1) in str(e.value) and e.value.code == bad[record][1]
        with pytest.raises(csv_ref.CsvError) as r:
            csv_ref.decode(text, _fields(I, D))
        assert r.value.record == record + 1
        lines[record] = b"0,0"
        text = b"\n".join(lines) + b"\n"
    _check(ctx, text, _fields(I, D))
    with pytest.raises(FlockGpuError) as e:
        ctx.csv_decode(_dev_bytes(b"1;2\n"), _fields(I, I), delimiter='"', has_header=False)
    assert e.value.code == _ffi.ERR_INVALID


# ---- the text at the end of a mapping ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", range(1, 34))
def test_text_ends_at_the_end_of_its_buffer(ctx, length):
    """Lengths of 1..33 bytes mod 16 and beyond one chunk: the last partial 16-byte chunk is read byte by byte (under FLOCK_TEST_GUARDED=1 the text ends
    where mapped memory ends, and a read past it faults)."""
    body = b"1,ab\n22,\"c\"\"d\"\n-3,\n4,efgh\n" * 700
    for text in (body[:length], body[: length + 16 * 1024]):
        text = text[:-1] + b"5" if text.endswith((b"\r", b'"', b"-")) else text
        try:
            want = csv_ref.decode(text, _fields(I, S), has_header=False)
        except csv_ref.CsvError:
            continue                                    # (a cut that leaves malformed text: not this test's subject)
        got, valid, n = ctx.csv_decode(_dev_bytes(text, at_end=True), _fields(I, S), has_header=False)
        _same(got, valid, n, *want, _fields(I, S))


# ---- q13 end to end ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_q13_from_a_csv_side_input(ctx):
    from flock_amd import NEXMarkSource, Window, run_query
    from flock_amd.nexmark import side_input_from_csv, synthetic_side_input
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_nexmark_goldens as m
    seed, eps, seconds = 31, 200_000, 3
    key, value = m.side_input_of(seed, eps, seconds, stride=61)
    text = ("key,value\n" + "".join("%d,%d\n" % kv for kv in zip(key.tolist(), value.tolist()))).encode()
    side = side_input_from_csv(ctx, _dev_bytes(text))
    assert np.array_equal(side[0].cpu().numpy(), key) and np.array_equal(side[1].cpu().numpy(), value) and len(key) > 100
    stream = NEXMarkSource(seconds, eps, Window.element_wise(), seed=seed).generate_data(ctx)
    want = run_query(ctx, 13, stream, side_input=synthetic_side_input(ctx, stream, stride=61)).to_host()
    got = run_query(ctx, 13, stream, side_input=side).to_host()
    assert sorted(got) == sorted(want) and len(want["value"]) > 0
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    with pytest.raises(ValueError):                     # the reference's fields are not nullable
        side_input_from_csv(ctx, _dev_bytes(b"key,value\n1,2\n3,\n"))


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_abi(ctx):
    from flock_amd import _ffi
    assert "flockgpu_csv_decode" in _ffi.SYMBOLS and hasattr(ctx._lib, "flockgpu_csv_decode")
    assert "int flockgpu_csv_decode(" in open(os.path.join(ROOT, "include", "flockgpu.h")).read()
    assert ctx._lib.flockgpu_abi_version() == 1
