"""Columns -> JSON lines / CSV on the GPU (flockgpu_json_lines_encode, flockgpu_csv_encode: textenc.hip) against tests/text_encode_ref.py, the reference of
textenc.hpp's A-ENC1..10 (itself checked against json.dumps, csv_ref and csv.reader in tests/test_text_encode_reference.py).  Every comparison is of the
bytes, exactly.  Generated relations and the round trip through both device decoders, row counts around the emit tile, source and output alignments,
class bytes on chunk and round seams, values that leave the LDS stage, the CSV specifics, every refusal, and the result buffer's contract."""
import numpy as np
import pytest

import oracle
import text_encode_ref as ref
from test_oracle_json import SCHEMAS, _events
from test_text_encode_reference import I, L, S, T, U, WEIRD, as_fields, corpus

pytestmark = pytest.mark.gpu

TILE = 256            # rows of an emit workgroup (textenc.hip kEncTile)
STAGE = 32 * 1024     # bytes of the emit pass's LDS stage = of a round (textenc.hip kEncStage)
TS_MIN, TS_MAX = ref.TS_MIN, ref.TS_MAX      # numtext.hpp kNumTextTsMin / kNumTextTsMax
ERR_INVALID, ERR_UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def ctx():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def _dev(columns, valid=None):
    """The reference's columns on the device: [(name, type, tensor | DeviceUtf8)], {name: uint8 tensor}."""
    from devmem import dev
    from flock_amd import DeviceUtf8
    cols = [(name, t, DeviceUtf8(dev(np.asarray(c.offsets, np.int32)), dev(np.asarray(c.data, np.uint8))) if t == S else dev(c)) for name, t, c in columns]
    return cols, {k: dev(v) for k, v in (valid or {}).items()}


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _check(ctx, columns, valid=None, formats=("json", "csv"), delimiter=b",", has_header=True):
    cols, dvalid = _dev(columns, valid)
    out = {}
    if "json" in formats:
        out["json"] = _bytes(ctx.json_lines_encode(cols, dvalid))
        assert out["json"] == ref.json_lines(columns, valid)
    if "csv" in formats:
        out["csv"] = _bytes(ctx.csv_encode(cols, dvalid, delimiter=delimiter, has_header=has_header))
        assert out["csv"] == ref.csv_text(columns, valid, delimiter=delimiter, has_header=has_header)
    return out


def _refused(code, words, call, *args, **kw):
    from flock_amd import FlockGpuError
    with pytest.raises(FlockGpuError) as e:
        call(*args, **kw)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


# ---- generated relations -----------------------------------------------------------------------------------------------------------------------------------------
def _same_decoded(got, cols, schema):
    for name, t in schema:
        if t == "utf8":
            off = got[name].offsets.cpu().numpy()
            assert np.array_equal(off, cols[name].offsets), name
            assert np.array_equal(got[name].data.cpu().numpy()[: off[-1]], cols[name].data[: off[-1]]), name
        else:
            assert np.array_equal(got[name].cpu().numpy(), cols[name]), name


@pytest.mark.parametrize("relation", ["bid", "auction", "person"])
def test_generated_relations(ctx, relation):
    from flock_amd.nexmark import columns_to_event_bytes, event_bytes_to_columns
    cols, schema = _events(relation), SCHEMAS[relation]
    n = len(cols[schema[0][0]])
    columns = [(name, t, cols[name]) for name, t in schema]
    dcols, _ = _dev(columns)
    want = oracle.nexmark_json_lines(relation, cols)
    text = ctx.json_lines_encode(dcols, borrow=True)
    assert _bytes(text) == want
    got, rows = ctx.json_lines_decode(text, schema)                   # the device text, in place
    assert rows == n
    _same_decoded(got, cols, schema)
    csv_fields = [(name, t) for name, t in schema]
    text = ctx.csv_encode(dcols, borrow=True)
    assert _bytes(text) == ref.csv_text(columns)
    got, valid, rows = ctx.csv_decode(text, csv_fields)
    assert rows == n and valid == {}
    _same_decoded(got, cols, schema)
    text = columns_to_event_bytes(ctx, relation, {name: c for name, _, c in dcols})
    assert _bytes(text) == want
    got, rows = event_bytes_to_columns(ctx, text, relation)
    assert rows == n
    _same_decoded(got, cols, schema)


def test_generated_bids_many_tiles(ctx):
    from flock_amd import Bids
    from flock_amd.nexmark import columns_to_event_bytes
    cols, schema = _events("bid", 300_000), SCHEMAS["bid"]
    n = len(cols["auction"])
    assert n > 64 * TILE
    columns = [(name, t, cols[name]) for name, t in schema]
    dcols, _ = _dev(columns)
    want = oracle.nexmark_json_lines("bid", cols)
    text = columns_to_event_bytes(ctx, "bid", Bids(*(c for _, _, c in dcols), n), borrow=True)
    assert _bytes(text) == want
    starts = np.flatnonzero(np.frombuffer(want, np.uint8) == 10)[TILE - 1::TILE] + 1          # where the tiles after the first begin
    assert len(set((starts % 16).tolist())) == 16                                               # every output alignment
    got, rows = ctx.json_lines_decode(text, schema)
    assert rows == n
    _same_decoded(got, cols, schema)
    assert _bytes(ctx.csv_encode(dcols)) == ref.csv_text(columns)


# ---- row counts around the tile -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [0, 1, TILE - 1, TILE, TILE + 1, 4 * TILE + 1])
def test_row_counts_around_the_tile(ctx, n_rows):
    columns, valid = corpus(11, n_rows=n_rows, types=[S, I, L, U, T, S, T, I])
    valid = {name: (np.arange(n_rows) % 3 != (k % 3)).astype(np.uint8) for k, (name, _, _) in enumerate(columns)}      # NULLs in every type
    got = _check(ctx, columns, valid)
    if n_rows == 0:
        assert got["json"] == b"" and got["csv"].count(b"\n") == 1
    # a validity pointer with no NULL behind it changes nothing
    cols, ones = _dev(columns, {name: np.ones(n_rows, np.uint8) for name, _, _ in columns})
    assert _bytes(ctx.json_lines_encode(cols, ones)) == _bytes(ctx.json_lines_encode(cols))
    assert _bytes(ctx.csv_encode(cols, ones, delimiter="|")) == _bytes(ctx.csv_encode(cols, delimiter="|")) == ref.csv_text(columns, delimiter=b"|")


@pytest.mark.parametrize("seed", range(3))
def test_seeded_corpus(ctx, seed):
    columns, valid = corpus(seed, n_rows=700)
    out = _check(ctx, columns, valid, delimiter=b"|" if seed & 1 else b",", has_header=seed != 2)
    cols, dvalid = _dev(columns, valid)
    got, got_valid, n = ctx.csv_decode(ctx.csv_encode(cols, dvalid, borrow=True), as_fields(columns))       # the identity on everything but NULL text
    assert n == 700 and out["csv"].count(b"\n") >= 700
    for name, t, col in columns:
        ok = valid.get(name, np.ones(700, np.uint8))
        if t == S:
            want = ref.utf8_of([s if ok[i] else b"" for i, s in enumerate(ref.strings_of(col))])
            off = got[name].offsets.cpu().numpy()
            assert np.array_equal(off, want.offsets) and np.array_equal(got[name].data.cpu().numpy()[: off[-1]], want.data), name
        else:
            assert (name in got_valid) == (not ok.all()) and (ok.all() or np.array_equal(got_valid[name].cpu().numpy(), ok)), name
            assert np.array_equal(got[name].cpu().numpy()[ok != 0], col[ok != 0]), name


# ---- alignment and seams --------------------------------------------------------------------------------------------------------------------------------------------
def test_every_source_and_output_alignment(ctx):
    values = [bytes([97 + (i + k) % 26 for k in range(n)]) for i, n in enumerate(list(range(41)) * 3)]       # lengths 0..40 in sequence
    begins = np.cumsum([0] + [len(v) for v in values])[:-1]
    assert len(set((begins % 16).tolist())) == 16
    out = _check(ctx, [("s", S, ref.utf8_of(values)), ("i", I, np.arange(len(values), dtype=np.int32) * 37)])
    for text in out.values():         # (no value holds a newline: every '\n' ends a row)
        row_begins = np.flatnonzero(np.frombuffer(text, np.uint8) == 10) + 1
        assert len(set((row_begins % 16).tolist())) == 16


@pytest.mark.parametrize("byte", [b'"', b"\x01", b"\n"])
def test_class_byte_on_a_chunk_seam(ctx, byte):
    values = []
    for at in (15, 16, 17):          # byte `at` of a source chunk: the values are laid out back to back, 48 bytes each
        values.append(b"a" * at + byte + b"b" * (47 - at))
    values += [b"c" * 48, byte, byte * 3 + b"d" * 45]
    _check(ctx, [("s", S, ref.utf8_of(values))])
    _check(ctx, [("n", L, np.arange(6, dtype=np.int64) - 3), ("s", S, ref.utf8_of(values))], {"s": np.array([1, 1, 0, 1, 1, 1], np.uint8)})


def test_a_value_of_control_bytes_grows_six_times(ctx):
    values = [b"\x01" * 37, b"", b"\x01", b"\x1f" * 700, b"\x00\x01\x02"]
    out = _check(ctx, [("s", S, ref.utf8_of(values))], has_header=False)
    assert len(out["json"].split(b"\n")[0]) == len(b'{"s":""}') + 6 * 37 and out["csv"].split(b"\n")[0] == b"\x01" * 37


def _long_value(n, classes, first, width):
    """n bytes whose class bytes sit where the emit pass's rounds meet.  `first`: where the value's first byte lands in the text; width(b): the bytes
    that b becomes.  The first tile's rounds meet at the multiples of STAGE of the text (a header is shorter than 16 bytes here); every source byte
    that lands within 8 bytes of one is a class byte, in turn: one ends just before the seam, one straddles or begins at it, one follows it."""
    v, pos, k = bytearray(), first, 0
    for _ in range(n):
        near = (pos + 8) % STAGE < 16 and pos > 100
        b = classes[k % len(classes)] if classes and near else 0x78
        k += near
        v.append(b)
        pos += width(b)
    return bytes(v), (pos - first) // STAGE


@pytest.mark.parametrize("fmt", ["json", "csv"])
@pytest.mark.parametrize("classes", [b'"\x01\n', b""], ids=["escaped", "verbatim"])
def test_a_value_longer_than_the_stage(ctx, classes, fmt):
    ints, stamps = np.array([7, -8, 9, 10, 11], np.int32), np.array([0, 1, TS_MAX, TS_MIN, 999], np.int64)
    valid = {"t": np.array([1, 1, 1, 1, 0], np.uint8)}
    for shift in (0, 5, 13):          # the bytes in front of the long value move every seam
        def table(values, rows=5):
            return [("i", I, ints[:rows]), ("s", S, ref.utf8_of(values[:rows])), ("t", T, stamps[:rows])]
        if fmt == "json":
            first = len(ref.json_lines(table([b"p" * shift], 1))) + len(b'{"i":-8,"s":"')
            width = lambda b: len(ref.json_string(bytes([b]))) - 2
        else:
            first = len(ref.csv_text(table([b"p" * shift], 1))) + len(b'-8,"' if classes else b"-8,")
            width = lambda b: 2 if b == 0x22 else 1
        long, seams = _long_value(3 * STAGE + 1234, classes, first, width)
        assert len(long) > STAGE and seams >= 3
        out = _check(ctx, table([b"p" * shift, long, b"after", b'q"', b""]), valid, formats=(fmt,))
        for k in range(1, seams + 1):          # the text around every seam is what the value was built to put there
            around = out[fmt][k * STAGE - 8:k * STAGE + 8]
            assert (around.count(b"\\u0001") + around.count(b"\\n") + around.count(b'""') > 0) == bool(classes), (k, around)


def test_a_row_of_64_columns(ctx):
    types = [(S, I, L, U, T)[k % 5] for k in range(64)]
    columns, valid = corpus(5, n_rows=TILE + 44, types=types, long_ok=False)
    assert len(columns) == 64
    _check(ctx, columns, valid)


# ---- CSV specifics ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_csv_delimiter_decides_the_quotes(ctx):
    columns = [("a|b", S, ref.utf8_of([b"x|y", b"x,y", b"", b'say "hi"', b"plain"])), ("n,m", I, np.arange(5, dtype=np.int32))]
    out = _check(ctx, columns, formats=("csv",), delimiter=b"|")
    assert out["csv"] == b'"a|b"|n,m\n"x|y"|0\nx,y|1\n""|2\n"say ""hi"""|3\nplain|4\n'
    out = _check(ctx, columns, formats=("csv",), delimiter=b",")
    assert out["csv"].startswith(b'a|b,"n,m"\nx|y,0\n"x,y",1\n')
    _check(ctx, [(WEIRD, S, ref.utf8_of([b"v"])), ('"', I, np.array([1], np.int32)), ("line\nbreak", L, np.array([2], np.int64))])


@pytest.mark.parametrize("t", [S, I, L, U, T])
def test_csv_one_column_null(ctx, t):
    col = ref.utf8_of([b"a", b"", b"b", b""]) if t == S else np.array([1, 2, 3, 4], np.int32 if t == I else np.int64)
    valid = {"c": np.array([1, 0, 1, 1], np.uint8)}
    out = _check(ctx, [("c", t, col)], valid, has_header=False)
    assert out["csv"].split(b"\n")[1] == b'""' and b"\n\n" not in out["csv"]
    cols, dvalid = _dev([("c", t, col)], valid)
    got, got_valid, n = ctx.csv_decode(ctx.csv_encode(cols, dvalid, has_header=False, borrow=True), [("c", t)], has_header=False)
    assert n == 4 and (t == S or got_valid["c"].cpu().numpy().tolist() == [1, 0, 1, 1])


def test_csv_timestamps_at_the_edges(ctx):
    ts = np.array([TS_MIN, TS_MAX, -1, 999, 1000, 0, 1_436_918_400_000], np.int64)
    out = _check(ctx, [("t", T, ts), ("same", L, ts)])
    assert out["csv"].split(b"\n")[1:4] == [b"0000-01-01 00:00:00,%d" % TS_MIN, b"9999-12-31 23:59:59.999,%d" % TS_MAX, b"1969-12-31 23:59:59.999,-1"]
    cols, _ = _dev([("t", T, ts)])
    got, valid, n = ctx.csv_decode(ctx.csv_encode(cols, borrow=True), [("t", T)])
    assert n == len(ts) and valid == {} and np.array_equal(got["t"].cpu().numpy(), ts)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(ctx):
    import torch
    col = torch.zeros(8, dtype=torch.int64, device="cuda")
    for encode in (ctx.json_lines_encode, ctx.csv_encode):
        _refused(ERR_UNSUPPORTED, ("Float64", "'f'", "column 1"), encode, [("a", L, col), ("f", "float64", col.view(torch.float64))])
        _refused(ERR_UNSUPPORTED, ("more than 64 columns", "column 64", "'c64'"), encode, [("c%d" % k, L, col) for k in range(65)])
        _refused(ERR_UNSUPPORTED, ("column 1", "1 to 31 bytes", "32"), encode, [("a", L, col), ("x" * 32, L, col)])
        _refused(ERR_UNSUPPORTED, ("1 to 31 bytes",), encode, [("", L, col)])
        _refused(ERR_INVALID, ("no columns",), encode, [])
        assert _bytes(encode([("x" * 31, L, col[:1])])).count(b"x") == 31
    _refused(ERR_INVALID, ("delimiter", "0x22"), ctx.csv_encode, [("a", L, col)], delimiter='"')
    _refused(ERR_INVALID, ("delimiter",), ctx.csv_encode, [("a", L, col)], delimiter="\n")


@pytest.mark.parametrize("header", [True, False])
def test_csv_timestamp_out_of_range_names_the_first_row(ctx, header):
    from devmem import dev
    ts = np.arange(1000, dtype=np.int64) * 1000
    ts[699], ts[299] = TS_MAX + 1, TS_MIN - 1                          # rows 700 and 300
    valid = np.ones(1000, np.uint8)
    columns = [("a", L, ts), ("when", T, ts)]
    cols, dvalid = _dev(columns, {"when": valid})
    with pytest.raises(ref.EncodeError) as e:
        ref.csv_text(columns, {"when": valid}, has_header=header)
    assert e.value.record == (301 if header else 300)
    _refused(ERR_INVALID, ("record %d:" % e.value.record, "column 1", "'when'", "0000 to 9999"), ctx.csv_encode, cols, dvalid, has_header=header)
    assert _bytes(ctx.json_lines_encode(cols, dvalid)) == ref.json_lines(columns, {"when": valid})       # JSON prints the integer
    valid[[299, 699]] = 0                                                # a NULL is not looked at
    assert _bytes(ctx.csv_encode(cols, {"when": dev(valid)}, has_header=header)) == ref.csv_text(columns, {"when": valid}, has_header=header)


def test_an_output_of_two_gib_is_refused_without_an_emit_launch(ctx):
    import torch
    col = torch.full((2**21,), -2**63, dtype=torch.int64, device="cuda")      # 16 MB; 64 aliases of it come to ~2.8 GB as CSV and more as JSON
    columns = [("c%d" % k, L, col) for k in range(64)]
    three = np.full(3, -2**63, np.int64)
    small = [("c0", L, three), ("c1", L, three)]
    ctx.profile(True)
    try:
        for encode, want in ((ctx.csv_encode, ref.csv_text(small)), (ctx.json_lines_encode, ref.json_lines(small))):
            ctx.profile_reset()
            _refused(ERR_UNSUPPORTED, ("2^31 - 16",), encode, columns)
            seen = ctx.profile_read()
            assert "textenc_len_kernel" in seen and "textenc_emit_kernel" not in seen, sorted(seen)
            assert _bytes(encode([(name, t, col[:3]) for name, t, _ in small])) == want          # the next call on the context succeeds
    finally:
        ctx.profile(False)


# ---- the result buffer -----------------------------------------------------------------------------------------------------------------------------------------------------
def test_result_buffer_contract(ctx):
    import ctypes as C

    from flock_amd import _ffi
    columns, valid = corpus(2, n_rows=333)
    cols, dvalid = _dev(columns, valid)
    for encode, want in ((ctx.json_lines_encode, ref.json_lines(columns, valid)), (ctx.csv_encode, ref.csv_text(columns, valid))):
        copy = encode(cols, dvalid)
        view = encode(cols, dvalid, borrow=True)                         # a second call on the context
        assert _bytes(copy) == _bytes(view) == want and view.numel() == len(want)
        assert view.data_ptr() % 16 == 0
        padded = (len(want) + 15) // 16 * 16
        tail = np.empty(padded - len(want), np.uint8)
        if len(tail):
            ctx._check(ctx._lib.flockgpu_memcpy(ctx._h, tail.ctypes.data_as(C.c_void_p), view.data_ptr() + len(want), len(tail), _ffi.D2H))
        assert not tail.any()
    for n_rows in (1, 2, 3, 5, 16):                                      # short texts: the zeros behind them, at several lengths
        view = ctx.json_lines_encode([("k", I, _dev([("k", I, np.arange(n_rows, dtype=np.int32))])[0][0][2])], borrow=True)
        n = view.numel()
        tail = np.empty((n + 15) // 16 * 16 - n, np.uint8)
        if len(tail):
            ctx._check(ctx._lib.flockgpu_memcpy(ctx._h, tail.ctypes.data_as(C.c_void_p), view.data_ptr() + n, len(tail), _ffi.D2H))
        assert _bytes(view) == b"".join(b'{"k":%d}\n' % k for k in range(n_rows)) and not tail.any()
