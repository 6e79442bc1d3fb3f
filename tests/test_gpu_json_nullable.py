"""JSON lines -> columns with NULLs on the GPU (flockgpu_json_lines_decode_nullable, json.hip A-JSONN1..7) against tests/json_nullable_ref.py (itself held
against json.loads and float() in tests/test_json_nullable_reference.py).  Every comparison is exact: values (Float64 by its bits), validity bytes, null
counts, offsets and bytes; for a refused text the status, the line and the message.  The sizes are the smallest at which the kernels can still go wrong:
both sides of the 256 lines of a workgroup, both placements of a workgroup's lines (staged in LDS or read from global memory), the field counts around
the unrolled instances."""
import ctypes as C
import re
import struct

import numpy as np
import pytest

import json_nullable_ref as ref
import json_ref
import test_json_nullable_reference as corp
from test_gpu_json_edges import LINES, _dev_bytes, _release, _unstaged, is_staged
from test_json_nullable_reference import ABSENT, D, FIELDS, I, L, S, T, U, write

pytestmark = pytest.mark.gpu

KINDS = {I: 0, L: 1, U: 2, D: 3, T: 4, S: 5}           # FLOCKGPU_TEXT_*
WIDTH = {I: (np.int32, "<i4"), L: (np.int64, "<i8"), U: (np.uint64, "<i8"), D: (np.float64, "<i8"), T: (np.int64, "<i8")}


@pytest.fixture(scope="module")
def ctx():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


@pytest.fixture()
def fresh():
    """a context of its own: the route hints are per context, and a test that names the kernels it expects starts from none"""
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def _raw(ctx, t, fields):
    """The C entry point itself -> (columns as the reference has them, validity bytes of EVERY nullable field, null counts, rows)."""
    import torch
    from flock_amd import _ffi
    fields = ref.normalise(fields)
    spec = (_ffi.JsonNField * len(fields))(*[_ffi.JsonNField(n.encode(), KINDS[ty], 1 if nl else 0) for n, ty, nl in fields])
    cols = (_ffi.JsonNColumn * len(fields))()
    rows = C.c_int64(-1)
    ctx._check(ctx._lib.flockgpu_json_lines_decode_nullable(ctx._h, t.data_ptr(), t.numel(), spec, len(fields), cols, C.byref(rows)))
    n, out, valid, nulls = rows.value, {}, {}, {}
    for (name, ty, nl), c in zip(fields, cols):
        if ty == S:
            off = ctx._device_view(c.utf8.offsets, n + 1, torch.int32).cpu().numpy() if n else np.zeros(1, np.int32)
            out[name] = (off, ctx._device_view(c.utf8.data, int(c.utf8_bytes), torch.uint8).cpu().numpy())
            assert c.values is None and int(c.utf8_bytes) == int(off[-1])
        else:
            dtype, _ = WIDTH[ty]
            g = ctx._device_view(c.values, n, torch.int32 if ty == I else torch.int64).cpu().numpy()
            out[name] = g.view(dtype)
        assert (c.valid is not None) == (nl and n > 0), name                     # written for every nullable field, and for no other
        if nl:
            valid[name] = ctx._device_view(c.valid, n, torch.uint8).cpu().numpy() if n else np.zeros(0, np.uint8)
        nulls[name] = int(c.null_count)
    return out, valid, nulls, n


def _same(got, want, fields):
    (g_cols, g_valid, g_nulls, n), (w_cols, w_valid, w_nulls) = got, want
    assert g_nulls == w_nulls
    assert sorted(g_valid) == sorted(w_valid)
    for name, ty, _ in ref.normalise(fields):
        if name in w_valid:
            assert np.array_equal(g_valid[name], w_valid[name]), name
        if ty == S:
            off, data = g_cols[name]
            assert len(off) == n + 1 and np.array_equal(off, w_cols[name].offsets), name
            assert np.array_equal(data[: off[-1]], w_cols[name].data), name
        else:
            g, w = g_cols[name], w_cols[name]
            assert g.dtype == w.dtype and len(g) == n, name
            assert np.array_equal(g.view(np.int64) if ty == D else g, w.view(np.int64) if ty == D else w), name   # (Float64 by its bits: -0.0 is not 0.0)


def _check(ctx, text, fields, want=None):
    want = want or ref.decode(text, fields)
    t = _dev_bytes(text)
    got = _raw(ctx, t, fields)
    _release(t)
    _same(got, want, fields)
    return got


def _refusal(ctx, text, fields):
    """(status, line, message) of the device's refusal of `text`."""
    from flock_amd import FlockGpuError, _ffi
    t = _dev_bytes(text)
    with pytest.raises(FlockGpuError) as e:
        _raw(ctx, t, fields)
    _release(t)
    msg = str(e.value)
    assert e.value.code in (_ffi.ERR_INVALID, _ffi.ERR_UNSUPPORTED), msg
    m = re.search(r"json: line (\d+): (.*)$", msg)
    assert m, msg
    return "unsupported" if e.value.code == _ffi.ERR_UNSUPPORTED else "invalid", int(m.group(1)), m.group(2)


def _agree(ctx, text, fields):
    """The device and the reference on any text: the same columns, or the same refusal.  -> the reference's error code, None for an accepted text."""
    try:
        want = ref.decode(text, fields)
    except ref.JsonError as r:
        assert _refusal(ctx, text, fields) == (r.status, r.line, r.message), text[-300:]
        return r.code
    _check(ctx, text, fields, want)
    return None


def _kernels(ctx, fn):
    """the kernels that ran during fn()"""
    ctx.profile_reset()
    ctx.profile(True)
    try:
        fn()
        return set(ctx.profile_read())
    finally:
        ctx.profile(False)


def _among_good(bad, fields, good, at=3):
    lines = [good] * 4
    lines.insert(at - 1, bad)
    return b"\n".join(lines) + b"\n"


def _both_placements(text):
    """the text as it is (its first workgroup staged in LDS) and with that workgroup read from global memory"""
    moved = _unstaged(text)
    assert is_staged(text) and not is_staged(moved)
    return (text, moved)


# ---- every type x {value, null, absent}, three writers, both placements ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("writer", [0, 1, 2])
def test_types_states_writers_placements(ctx, writer):
    lines = []
    for k, (name, ty) in enumerate(FIELDS * 2):                                          # each field in each state, the others holding values
        for state in ("value", None, ABSENT):
            rng = np.random.default_rng(k)
            items = [(n, corp.a_value(rng, t, k + j) if n != name or state == "value" else state) for j, (n, t) in enumerate(FIELDS)]
            lines.append(write(items, writer, len(lines)))
    lines = [write([(n, 1 if t != S else "x") for n, t in FIELDS], writer)] + lines + corp.corpus(writer, 300 - len(lines), writers=(writer,))
    text = b"\n".join(lines) + b"\n"
    want = ref.decode(text, FIELDS)
    assert all(0 < want[2][n] < len(lines) for n, _ in FIELDS)
    for placed in _both_placements(text):
        _check(ctx, placed, FIELDS, want)
    _check(ctx, text[:-1], FIELDS, want)                                                  # and without the last newline


# ---- null in the compact walker -------------------------------------------------------------------------------------------------------------------------------------
ABC = [("a", L), ("b", S), ("c", I)]


def test_null_stays_with_the_compact_walker(fresh):
    """null as the first, a middle and the last field of a compact line, two in a row, all three: every line is parse_line_words', no workgroup is flagged and
    the second kernel does not run."""
    ctx = fresh
    shapes = [b'{"a":null,"b":"x","c":3}', b'{"a":1,"b":null,"c":3}', b'{"a":1,"b":"x","c":null}', b'{"a":null,"b":null,"c":3}',
              b'{"a":1,"b":null,"c":null}', b'{"a":null,"b":null,"c":null}', b'{"a":-7,"b":"","c":0}']
    text = b"\n".join(shapes * 43) + b"\n"                                                # 301 lines: two workgroups
    ran = _kernels(ctx, lambda: _check(ctx, text, ABC))
    assert "json_nparse_kernel" in ran and "json_null_count_kernel" in ran and "json_nparse_retry_kernel" not in ran, sorted(ran)
    got = _check(ctx, text, ABC)
    assert got[2] == {"a": 3 * 43, "b": 4 * 43, "c": 3 * 43}
    plain = {I: -2147483648, L: 999999999999999999, U: 18446744073709551615, D: b"#123456.789e3", T: 1_600_000_000_000, S: "café"}   # what that walker takes
    six = b"\n".join(write([(n, None if (k >> j) & 1 else plain[t]) for j, (n, t) in enumerate(FIELDS)], 0) for k in range(64)) + b"\n"   # every subset NULL
    ran = _kernels(ctx, lambda: _check(ctx, six, FIELDS))
    assert "json_nparse_retry_kernel" not in ran, sorted(ran)


def test_an_absent_member_takes_the_second_kernel(fresh):
    ctx = fresh
    text = b'{"a":1,"b":"x","c":3}\n' * 5 + b'{"a":1,"c":3}\n{"c":4,"a":null}\n{}\n { } \n'
    ran = _kernels(ctx, lambda: _check(ctx, text, ABC))
    assert "json_nparse_retry_kernel" in ran, sorted(ran)
    got = _check(ctx, _unstaged(text), ABC)
    assert got[2] == {"a": 3, "b": 4, "c": 2}


def test_empty_object(ctx):
    got = _check(ctx, b"{}\n", ABC)
    assert got[3] == 1 and got[2] == {"a": 1, "b": 1, "c": 1}
    _check(ctx, b"{}\n" * 300, FIELDS)
    req = [("a", L), ("b", S, False), ("c", I)]
    for placed in _both_placements(_among_good(b"{}", req, b'{"a":1,"b":"x","c":3}')):
        assert _refusal(ctx, placed, req) == ("invalid", 3, json_ref.MESSAGES["missing"])
    assert _refusal(ctx, b'{"b":"x"}\n\n{}\n', ABC) == ("unsupported", 2, json_ref.MESSAGES["blank"])     # a blank line stays refused
    assert _check(ctx, b"", ABC)[3] == 0


# ---- the seams of the parse kernel ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 512, 513])
def test_workgroup_seams(ctx, n):
    """NULLs on the last line of a workgroup and on the first line of the next; 257 and 513 lines leave the last workgroup one line."""
    assert LINES == 256
    edge = {LINES - 1, LINES, 2 * LINES - 1, 2 * LINES, n - 1}
    for shape in ("null", "absent"):
        lines = []
        for k in range(n):
            state = None if shape == "null" else ABSENT
            items = [(nm, state if k in edge else corp.a_value(np.random.default_rng(k), t, k + j)) for j, (nm, t) in enumerate(FIELDS)]
            lines.append(write(items, 0))
        text = b"\n".join(lines) + b"\n"
        got = _check(ctx, text, FIELDS)
        assert got[3] == n and all(v == len([k for k in edge if k < n]) for v in got[2].values())
        for name, _ in FIELDS:
            assert [k for k in range(n) if got[1][name][k] == 0] == sorted(k for k in edge if k < n)


# ---- field counts around the unrolled instances ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fields", [1, 4, 5, 8, 9, 16])
def test_field_counts(ctx, n_fields):
    types = [I, L, U, D, T, S]
    fields = [("f%02d" % f, types[f % 6]) for f in range(n_fields)]
    for writer in (0, 1, 2):
        lines = []
        for k in range(40):
            rng = np.random.default_rng(100 * n_fields + k)
            lines.append(write([(n, [None, ABSENT][k % 2] if (k + j) % 5 == 0 and k % 3 else corp.a_value(rng, t, k + j)) for j, (n, t) in enumerate(fields)], writer, k))
        _check(ctx, b"\n".join(lines) + b"\n", fields)


def test_seventeen_fields_are_refused(ctx):
    from flock_amd import FlockGpuError, _ffi
    fields = [("f%02d" % f, I) for f in range(17)]
    t = _dev_bytes(b"{}\n")
    with pytest.raises(FlockGpuError) as e:
        _raw(ctx, t, fields)
    with pytest.raises(FlockGpuError):
        ctx.json_lines_decode_nullable(t, fields)
    _release(t)
    assert e.value.code == _ffi.ERR_UNSUPPORTED and "json: more than 16 fields" in str(e.value)


# ---- numbers ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _number_lines(tok):
    """the token in a compact line, after a space with the members rotated, and in front of the closing brace"""
    return [b'{"k":1,"v":%s,"s":"x"}' % tok, b'{"s": "x", "v": %s , "k": 1}' % tok, b'{"k":1,"s":"x","v":%s}' % tok, b'{"k":1,"s":"x","zz":[],"v":%s }' % tok]


def _numbers(ctx, ty, accepted, refused):
    fields = [("k", I), ("v", ty), ("s", S)]
    good = b'{"k":1,"v":1,"s":"x"}'
    text = b"\n".join(line for tok in accepted for line in _number_lines(tok)) + b"\n"
    for placed in _both_placements(text):
        got = _check(ctx, placed, fields)
    for tok, status, code in refused:
        for line in _number_lines(tok):
            for placed in _both_placements(_among_good(line, fields, good)):
                want = (status, 3, ref.MESSAGES[code] % "v" if code == "float" else ref.MESSAGES[code])
                assert _refusal(ctx, placed, fields) == want, line
    return got


def test_uint64(ctx):
    got = _numbers(ctx, U, [b"0", b"9223372036854775807", b"9223372036854775808", b"18446744073709551615", b"18446744073709551614", b"10000000000000000000", b"1844674407370955161"],
                   [(b"18446744073709551616", "invalid", "range"), (b"18446744073709551620", "invalid", "range"), (b"184467440737095516150", "invalid", "range"),
                    (b"-0", "invalid", "range"), (b"-1", "invalid", "range"), (b"1e3", "unsupported", "number"), (b"01", "invalid", "malformed")])
    assert got[0]["v"][:16:4].tolist() == [0, (1 << 63) - 1, 1 << 63, (1 << 64) - 1]


def test_int64_and_timestamp_extremes(ctx):
    for ty in (L, T):
        _numbers(ctx, ty, [b"9223372036854775807", b"-9223372036854775808", b"-0", b"999999999999999999", b"-999999999999999999"],
                 [(b"9223372036854775808", "invalid", "range"), (b"-9223372036854775809", "invalid", "range"), (b"1.0", "unsupported", "number"),
                  (b'"2020-01-01 00:00:00"', "invalid", "malformed")])
    _numbers(ctx, I, [b"2147483647", b"-2147483648"], [(b"2147483648", "invalid", "range"), (b"true", "invalid", "malformed")])


def test_float64(ctx):
    accepted = [b"9007199254740992", b"1e22", b"1E-22", b"0.1", b"-0.0", b"3", b"123456.789e3", b"-0", b"0e999", b"0.000e-5", b"1.50", b"100e-2", b"-2.5E+3",
                b"1000000000000000000000", b"90071992547409920e-1", b"12345678901234.5", b"0.0000000000000000000001", b"4.9e-5"]
    got = _numbers(ctx, D, accepted,
                   [(b"9007199254740993", "unsupported", "float"), (b"1e23", "unsupported", "float"), (b"1e-23", "unsupported", "float"),
                    (b"0.12345678901234567", "unsupported", "float"), (b"1e400", "unsupported", "float"),
                    (b"+1", "invalid", "malformed"), (b"01", "invalid", "malformed"), (b".5", "invalid", "malformed"), (b"1.", "invalid", "malformed"),
                    (b"1e", "invalid", "malformed"), (b"1e+", "invalid", "malformed"), (b"nan", "invalid", "malformed"), (b"Infinity", "invalid", "malformed"),
                    (b"-Infinity", "invalid", "malformed"), (b'"1.5"', "invalid", "malformed"), (b"1e23x", "invalid", "malformed"), (b"false", "invalid", "malformed")])
    for k, tok in enumerate(accepted):                                                     # bit for bit what Python's float() gives
        assert all(struct.pack("<d", v) == struct.pack("<d", float(tok)) for v in got[0]["v"][4 * k:4 * k + 4]), tok
    rng = np.random.default_rng(5)
    toks = [t for t in (corp.float_token(rng) for _ in range(1500)) if ref.exact_f64(t) is not None][:600]
    text = b"\n".join(b'{"v":%s}' % t for t in toks) + b"\n"
    got = _check(ctx, text, [("v", D)])
    assert got[0]["v"].view(np.int64).tolist() == np.array([float(t) for t in toks]).view(np.int64).tolist()


def test_wrong_types_and_near_null_spellings(ctx):
    good = b'{"a":1,"b":"x","c":3}'
    req = [("a", L, False), ("b", S), ("c", I)]
    cases = [(b'{"a":true,"b":"x","c":3}', ABC), (b'{"a":1,"b":"x","c":false}', ABC), (b'{"a":1,"b":7,"c":3}', ABC), (b'{"a":"1","b":"x","c":3}', ABC),
             (b'{"a":nul,"b":"x","c":3}', ABC), (b'{"a":NULL,"b":"x","c":3}', ABC), (b'{"a":nullx,"b":"x","c":3}', ABC), (b'{"a":1,"b":"x","c":nul}', ABC),
             (b'{"a":1,"b":nullx,"c":3}', ABC), (b'{"a":1,"b":"x","c":nullx}', ABC), (b'{"a": null x, "b": "x", "c": 3}', ABC), (b'{"a":1,"b":"x","c":null', ABC),
             (b'{"a":null,"b":"x","c":3}', req), (b'{"c":3,"b":"x", "a" : null}', req)]          # null for a required field: the first entry point's message
    for bad, fields in cases:
        for placed in _both_placements(_among_good(bad, fields, good)):
            assert _refusal(ctx, placed, fields) == ("invalid", 3, json_ref.MESSAGES["malformed"]), bad
    ts = [("t", T), ("b", S)]
    assert _refusal(ctx, _among_good(b'{"t":"2020-01-01 00:00:00","b":"x"}', ts, b'{"t":1,"b":"x"}'), ts) == ("invalid", 3, json_ref.MESSAGES["malformed"])
    _check(ctx, good + b"\n", ABC)                                                        # afterwards the context decodes a good text


@pytest.mark.parametrize("writer", [0, 1, 2])
def test_repeated_keys(ctx, writer):
    """the last occurrence wins, and every occurrence is checked and typed"""
    rows = [[("a", 1), ("a", None), ("b", "x"), ("c", 3)], [("a", None), ("a", 1), ("b", "x"), ("c", 3)], [("a", 1), ("b", "x"), ("b", None), ("c", None), ("c", 5)],
            [("b", None), ("a", 2), ("b", "y\n"), ("b", None), ("c", 1)], [("a", 1), ("b", "x"), ("c", 3)]]
    text = b"\n".join(write(r, writer, k) for k, r in enumerate(rows * 60)) + b"\n"
    want = ref.decode(text, ABC)
    assert want[2]["a"] > 0 and len(want[1]["a"]) == 300                                 # (writer 1 rotates the members: which occurrence is last differs by line)
    for placed in _both_placements(text):
        _check(ctx, placed, ABC, want)
    bad = write([("a", 1), ("b", "x"), ("c", b"#1.5"), ("c", None)], writer)
    assert _refusal(ctx, _among_good(bad, ABC, write(rows[4], writer)), ABC) == ("unsupported", 3, json_ref.MESSAGES["number"])


def test_first_offender(ctx):
    """A-JSON8: the first offending line is named, whichever kernel or lane met one first"""
    fields = [("v", D), ("s", S)]
    good, declined, broken = b'{"v":0.5,"s":null}', b'{"v":1e23,"s":"x"}', b'{"v":0.5,"s":nul}'
    for first, second, want in ((declined, broken, ("unsupported", ref.MESSAGES["float"] % "v")), (broken, declined, ("invalid", ref.MESSAGES["malformed"]))):
        for a, b in ((3, 4), (10, 700), (256, 257), (300, 301)):
            lines = [good] * 800
            lines[a - 1], lines[b - 1] = first, second
            text = b"\n".join(lines) + b"\n"
            assert _refusal(ctx, text, fields) == (want[0], a, want[1])
            assert _agree(ctx, text, fields) is not None


# ---- the encoder's output read back ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 3001])
def test_round_trip_through_the_encoder(ctx, n):
    """json_lines_decode_nullable(json_lines_encode(cols, valid), fields) gives cols and valid back -- a NULL Utf8 and '' distinct, which CSV cannot do."""
    import torch
    from flock_amd.engine import DeviceUtf8
    r = np.random.default_rng(n)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    strings = [b"", b"plain", b'q"uote', b"back\\slash", b"\x01\x1f\t\n\r\x08\x0c", "café 漢".encode(), b"\xff\x80", b"null"]
    vals = [strings[int(x)] for x in r.integers(0, len(strings), n)]
    off = np.zeros(n + 1, np.int32)
    np.cumsum([len(v) for v in vals], out=off[1:])
    data = np.frombuffer(b"".join(vals) + b"\0" * 16, np.uint8).copy()
    host = {"i": r.integers(-2 ** 31, 2 ** 31, n).astype(np.int32), "l": r.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64),
            "u": r.integers(0, 2 ** 64 - 1, n, dtype=np.uint64).view(np.int64), "t": r.integers(-10 ** 15, 10 ** 15, n).astype(np.int64)}
    types = [("i", I), ("l", L), ("u", U), ("t", T), ("s", S)]
    holes = {name: (r.random(n) >= 0.2).astype(np.uint8) for name, _ in types if name != "l"}      # `l` holds no NULL
    if n:
        holes["s"][0] = 0                                                                           # a NULL Utf8 whatever the draw gives
    for name in host:                                                                               # (the decoder gives value 0 for a NULL)
        host[name] = np.where(holes[name] == 1, host[name], 0).astype(host[name].dtype) if name in holes else host[name]
    lens = np.where(holes["s"] == 1, off[1:] - off[:-1], 0)
    columns = [(name, ty, DeviceUtf8(dev(off), dev(data)) if ty == S else dev(host[name])) for name, ty in types]
    valid = {name: dev(v) for name, v in holes.items()}
    text = ctx.json_lines_encode(columns, valid, borrow=False)
    padded = torch.zeros((text.numel() + 31) // 16 * 16, dtype=torch.uint8, device=text.device)
    padded[: text.numel()] = text
    got, got_valid, rows = ctx.json_lines_decode_nullable(padded[: text.numel()], types)
    assert rows == n
    expect_valid = {name: v for name, v in holes.items() if n and (v == 0).any()}
    assert sorted(got_valid) == sorted(expect_valid) and "l" not in got_valid
    for name, v in expect_valid.items():
        assert np.array_equal(got_valid[name].cpu().numpy(), v), name
    for name in host:
        g = got[name].cpu().numpy()
        assert g.dtype == host[name].dtype and np.array_equal(g, host[name]), name
    g_off = got["s"].offsets.cpu().numpy()
    assert np.array_equal(g_off[1:] - g_off[:-1], lens)
    assert bytes(got["s"].data.cpu().numpy()[: g_off[-1]]) == b"".join(v for v, ok in zip(vals, holes["s"]) if ok)
    if n > 255:
        empty = [k for k in range(n) if lens[k] == 0]
        assert {int(holes["s"][k]) for k in empty} == {0, 1}                                        # NULL and '' both occur, and come back distinct
    borrowed, b_valid, _ = ctx.json_lines_decode_nullable(padded[: text.numel()], types, borrow=True)
    assert sorted(b_valid) == sorted(got_valid) and all(np.array_equal(borrowed[k].cpu().numpy(), host[k]) for k in host)


# ---- into a plan ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_decoded_text_with_nulls_feeds_a_plan(ctx):
    """COUNT(*), COUNT(x), SUM(x), MAX(t) WHERE s IS NOT NULL over the decoded columns equals the same rows fed as host Arrow batches"""
    import pyarrow as pa
    import device_feed_util as u
    import plan_corpus as pc
    from flock_amd.runtime import ExecutionContext
    fields = [("x", L), ("t", T), ("s", S), ("w", L)]
    r = np.random.default_rng(11)
    lines = []
    for k in range(3000):
        items = [("x", None if r.random() < 0.2 else int(r.integers(-10 ** 6, 10 ** 6))), ("t", ABSENT if r.random() < 0.1 else int(1_600_000_000_000 + r.integers(0, 10 ** 9))),
                 ("s", None if r.random() < 0.3 else ["", "a", "null"][k % 3]), ("w", k)]
        lines.append(write(items, 0 if k % 50 else 1, k))
    text = b"\n".join(lines) + b"\n"
    cols, valid, nulls = ref.decode(text, fields)
    assert nulls["w"] == 0 and min(nulls["x"], nulls["t"], nulls["s"]) > 100
    s = pc.scan([("x", "Int64"), ("t", "ts"), ("s", "Utf8"), ("w", "Int64")])
    plan = pc.aggregate(pc.filt(s, {"physical_expr": "is_not_null_expr", "arg": s.c("s")}), [], [("count", None), ("count", "x"), ("sum", "x"), ("max", "t")]).plan
    strings = [bytes(cols["s"].data[a:b]).decode() for a, b in zip(cols["s"].offsets[:-1], cols["s"].offsets[1:])]
    batch = pa.record_batch([pa.array(cols["x"], mask=valid["x"] == 0), pa.array(cols["t"], mask=valid["t"] == 0).cast(pa.timestamp("ms")),
                             pa.array(strings, mask=valid["s"] == 0), pa.array(cols["w"])], names=["x", "t", "s", "w"])
    t = _dev_bytes(text)
    run = ExecutionContext([plan], gpu=ctx)
    try:
        d_cols, d_valid, rows = ctx.json_lines_decode_nullable(t, fields, borrow=True)
        assert rows == 3000 and sorted(d_valid) == ["s", "t", "x"]                         # `w` reaches the leaf without validity
        assert run.feed_device_sources([([(name, ty, d_cols[name]) for name, ty in fields], d_valid)]) == 1
        dev = u.norm(u.batch_rows(run.execute()[0]))
        run.clean_data_sources()
        run.feed_data_sources([[[batch]]])
        host = u.norm(u.batch_rows(run.execute()[0]))
        run.clean_data_sources()
    finally:
        run.close()
        _release(t)
    keep = valid["s"] == 1
    assert dev == host and len(dev) == 1
    assert list(dev[0])[:3] == [int(keep.sum()), int((keep & (valid["x"] == 1)).sum()), int(cols["x"][keep].sum())]


# ---- seeded one-byte mutants of texts with nulls and absent members ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,count", corp.MUTANT_RUNS)
def test_mutant_differential(ctx, seed, count):
    """(tests/test_json_nullable_reference.py asserts, on the reference alone, that accepted and refused mutants are each at least a fifth of the corpus)"""
    codes = [_agree(ctx, corp.mutant_text(line), corp.MUTANT_FIELDS) for line in corp.mutants(seed, count)]
    assert None in codes and {"malformed", "missing"} <= set(codes)


# ---- the first entry point ------------------------------------------------------------------------------------------------------------------------------------------------
OLD_FIELDS = [("a", "int64"), ("b", "utf8")]
OLD_GOOD = b'{"a":1,"b":"x"}\n' * 599 + b'{"b": "after", "a": -2}\n'                      # three workgroups, one of them for the second kernel
SPACED = b'{"b": "x", "a": 1}\n' * 600                                                    # every workgroup takes the second kernel: the route hint flips
NEW_GOOD = b'{"a":null,"b":"x"}\n' * 599 + b'{"b":"y"}\n'                                 # likewise for the new entry: NULLs, and one absent member


def _first_entry(ctx, text=OLD_GOOD):
    t = _dev_bytes(text)
    got, n = ctx.json_lines_decode(t, OLD_FIELDS)
    _release(t)
    want = json_ref.decode(text, OLD_FIELDS)
    assert n == 600 and np.array_equal(got["a"].cpu().numpy(), want["a"]) and np.array_equal(got["b"].offsets.cpu().numpy(), want["b"].offsets)


def test_the_first_entry_point_is_untouched_by_calls_of_the_second(fresh):
    from flock_amd import FlockGpuError
    ctx = fresh
    for _ in range(3):
        _check(ctx, NEW_GOOD, OLD_FIELDS)
        _first_entry(ctx)
    # each entry point keeps a route hint of its own: spaced texts send the new entry straight to its second kernel ...
    for _ in range(3):
        ran = _kernels(ctx, lambda: _check(ctx, SPACED, OLD_FIELDS))
    assert "json_nparse_retry_kernel" in ran and "json_nparse_kernel" not in ran, sorted(ran)
    # ... and the first entry still starts a compact text with its first kernel
    ran = _kernels(ctx, lambda: _first_entry(ctx))
    assert "json_parse_kernel" in ran and not any(k.startswith("json_nparse") or k == "json_null_count_kernel" for k in ran), sorted(ran)
    for bad, message in ((b'{"a":null,"b":"x"}', "malformed JSON"), (b'{"b":"x"}', "a schema field is missing")):   # and refuses what it always refused
        t = _dev_bytes(b'{"a":1,"b":"x"}\n' + bad + b"\n")
        with pytest.raises(FlockGpuError, match="json: line 2: " + message):
            ctx.json_lines_decode(t, OLD_FIELDS)
        _release(t)
        _check(ctx, b'{"a":1,"b":"x"}\n' + bad + b"\n", OLD_FIELDS)                        # the same text is two rows for the new entry


def test_the_second_entry_point_is_untouched_by_the_route_of_the_first(fresh):
    ctx = fresh
    for _ in range(3):
        ran = _kernels(ctx, lambda: _first_entry(ctx, SPACED))
        _check(ctx, NEW_GOOD, OLD_FIELDS)
    assert "json_parse_retry_kernel" in ran and "json_parse_kernel" not in ran, sorted(ran)
    ran = _kernels(ctx, lambda: _check(ctx, NEW_GOOD[:-10], OLD_FIELDS))                   # (without the line that lacks a member)
    assert "json_nparse_kernel" in ran and "json_nparse_retry_kernel" not in ran, sorted(ran)
