"""JSON lines -> columns on the GPU (flockgpu_json_lines_decode, json.hip) against tests/json_ref.py, the reference of json.hip's A-JSON1..9 (itself checked
against json.loads in tests/test_json_reference.py).  Every comparison is exact: values, offsets, bytes, and for a refused text the status, the line number
and the message.  Every error with its line in both placements of its workgroup (staged in LDS or not), the well-formed edges, the schema's limits, bytes
crafted onto the seams of the line index and of the stage, the first offender among many lines on both routes, the route hint over 40 calls, the text at
the end of its buffer, and a seeded one-byte mutant differential."""
import ctypes as C
import re

import numpy as np
import pytest

import json_ref
from test_json_reference import AB, ERRORS, GOOD, MUTANT_FIELDS, WELL_FORMED, mutant_text, mutants

pytestmark = pytest.mark.gpu

I, L, S = "int32", "int64", "utf8"
# json.hip's constants, restated (tests/test_source_constants.py holds them against the source)
TILE = 256 * 64                 # kNlTile: bytes per tile of the line index; a lane's 64 bytes, a wave's 4 KiB
LINES = 256                     # kParseLines: lines per workgroup
STAGE_MAX = 48 * 1024           # kStageBytes


def stage_bytes(n_bytes, n_lines):
    want = (n_bytes // max(n_lines, 1) + 1) * LINES * 5 // 4 + 64
    return min(STAGE_MAX, (want + 1023) & ~1023)


def block_span(text, block):
    """b1 - a0 + 16 of workgroup `block`: what json_parse_kernel holds against stage_bytes."""
    starts = [0] + [m.end() for m in re.finditer(b"\n", text)]
    n_lines = len(starts) - (1 if text.endswith(b"\n") else 0)
    starts = starts[:n_lines] + [len(text)]
    b0, b1 = starts[block * LINES], starts[min((block + 1) * LINES, n_lines)]
    return b1 - (b0 & ~15) + 16, stage_bytes(len(text), n_lines)


def is_staged(text, block=0):
    span, stage = block_span(text, block)
    return span <= stage


@pytest.fixture(scope="module")
def ctx():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def _dev_bytes(b, at_end=False):
    """The text on the device, 16-byte aligned.  at_end: it ENDS where the allocation's 16-byte granule ends (and where mapped memory ends under
    FLOCK_TEST_GUARDED=1, tests/test_gpu_guard.py): nothing lies behind the last partial 16-byte chunk but that chunk's own padding."""
    from devmem import dev, guarded
    if guarded():
        return dev(np.frombuffer(bytes(b), np.uint8))
    import torch
    t = torch.zeros((len(b) + 15) // 16 * 16 + (0 if at_end else 16), dtype=torch.uint8, device="cuda")
    if len(b):
        t[: len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    return t[: len(b)]


def _release(t):
    """Under the guard every text is an allocation of its own that lives as long as its context: the tests that make thousands of calls hand theirs back."""
    import devmem
    if devmem.guarded():
        g = devmem._GUARD_CTX
        g._check(g._lib.flockgpu_free_guarded(g._h, C.c_void_p(t.data_ptr())))


def _same(got, n, want, fields):
    for name, t in fields:
        if t == S:
            off = got[name].offsets.cpu().numpy()
            assert len(off) == n + 1 and np.array_equal(off, want[name].offsets), name
            assert np.array_equal(got[name].data.cpu().numpy()[: off[-1]], want[name].data), name
        else:
            g = got[name].cpu().numpy()
            assert g.dtype == want[name].dtype and len(g) == n and np.array_equal(g, want[name]), name


def _check(ctx, text, fields, want=None, at_end=False):
    want = want or json_ref.decode(text, fields)
    t = _dev_bytes(text, at_end)
    got, n = ctx.json_lines_decode(t, fields)
    _same(got, n, want, fields)
    _release(t)
    return got, n


def _refusal(ctx, text, fields, at_end=False):
    """(status, line, message) of the device's refusal of `text`."""
    from flock_amd import FlockGpuError, _ffi
    t = _dev_bytes(text, at_end)
    with pytest.raises(FlockGpuError) as e:
        ctx.json_lines_decode(t, fields)
    _release(t)
    msg = str(e.value)
    assert e.value.code in (_ffi.ERR_INVALID, _ffi.ERR_UNSUPPORTED), msg
    m = re.search(r"json: line (\d+): (.*)$", msg)
    assert m, msg
    return "unsupported" if e.value.code == _ffi.ERR_UNSUPPORTED else "invalid", int(m.group(1)), m.group(2)


def _agree(ctx, text, fields, at_end=False):
    """The device and the reference on any text: the same columns, or the same refusal.  -> the reference's error code, None for an accepted text."""
    try:
        want = json_ref.decode(text, fields)
    except json_ref.JsonError as r:
        assert _refusal(ctx, text, fields, at_end) == (r.status, r.line, json_ref.MESSAGES[r.code]), text[-200:]
        return r.code
    _check(ctx, text, fields, want, at_end)
    return None


def _unstaged(text):
    """The same lines with a member of 60 000 bytes, not in the schema, added to line 1: the workgroup's lines no longer fit the stage, and every lane reads
    its line from global memory (Text<false>)."""
    first = text.index(b"\n")
    assert text[first - 1:first] == b"}"
    out = text[:first - 1] + b',"pad":"' + b"p" * 60_000 + b'"}' + text[first:]
    assert not is_staged(out) and is_staged(text)
    return out


# ---- every error, with its line, in both placements ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(ERRORS)))
def test_errors(ctx, case):
    text, fields, (status, line, code) = ERRORS[case]
    for placed in (text, _unstaged(text)):
        assert _refusal(ctx, placed, fields) == (status, line, json_ref.MESSAGES[code]), placed[-300:]
        _check(ctx, GOOD + b"\n" + b'{"b": "after", "a": -2}\n', AB)          # afterwards the context decodes a good text


# ---- well-formed edges ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", [w[0] for w in WELL_FORMED])
def test_well_formed_edges(ctx, what):
    _, text, fields = next(w for w in WELL_FORMED if w[0] == what)
    want = json_ref.decode(text, fields)
    _, n = _check(ctx, text, fields, want)
    assert n == text.count(b"\n") > 8
    _check(ctx, _unstaged(text), fields, want)                                  # the same lines read from global memory
    _check(ctx, text[:-1], fields, want)                                        # and without the last newline


def test_integer_extremes_stay_with_the_compact_walker(ctx):
    """A text of which parse_line_words takes every line (no workgroup is flagged, the second kernel does not run): both ends of Int32, -0, and the
    longest Int64 that walker reads (18 digits)."""
    fields = [("i", I), ("l", L), ("s", S)]
    vals = [(2147483647, 999999999999999999), (-2147483648, -999999999999999999), (0, 0), (-1, 1), (2147483647, -1), (-2147483648, 100000000000000000)]
    lines = [b'{"i":%d,"l":%d,"s":"%s"}' % (i, l, b"x" * (k % 19)) for k, (i, l) in enumerate(vals * 100)] + [b'{"i":-0,"l":-0,"s":"\xc3\xa9"}'] * 7
    text = b"\n".join(lines) + b"\n"
    got, n = _check(ctx, text, fields)
    assert n == 607 and got["i"].cpu().tolist()[-1] == 0 and got["l"].cpu().tolist()[:2] == [999999999999999999, -999999999999999999]


# ---- limits -------------------------------------------------------------------------------------------------------------------------------------------------------------
def _write(items, writer, k):
    """One line of (name, value) members as one of three writers: 0 compact (parse_line_words), 1 a space after ':' and ',' with the members rotated
    (parse_line_flex), 2 compact with a member that is not in the schema (parse_line)."""
    val = lambda v: b"%d" % v if isinstance(v, int) else b'"' + v + b'"'
    if writer == 1:
        items = items[k % len(items):] + items[:k % len(items)]
        return b"{" + b", ".join(b'"%s": %s' % (nm.encode(), val(v)) for nm, v in items) + b"}"
    body = [b'"%s":%s' % (nm.encode(), val(v)) for nm, v in items]
    if writer == 2:
        body.insert(k % (len(body) + 1), b'"not in the schema":[%d,{"k":"}"}]' % k)
    return b"{" + b",".join(body) + b"}"


def _rows(fields, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        out.append([(nm, int(rng.integers(-2 ** 31, 2 ** 31)) if t == I else int(rng.integers(-2 ** 62, 2 ** 62)) if t == L else b"v%d/%s" % (k, nm.encode()[:k % 9])) for nm, t in fields])
    return out


def _three_writers(ctx, fields, n=600, seed=1):
    rows = _rows(fields, n, seed)
    want = None
    for writer in range(3):
        text = b"\n".join(_write(r, writer, k) for k, r in enumerate(rows)) + b"\n"
        want = want or json_ref.decode(text, fields)                            # (the same rows whoever wrote them)
        _check(ctx, text, fields, want)
    return rows


@pytest.mark.parametrize("lengths", [range(1, 9), range(9, 17), range(17, 25), range(25, 32)], ids=["1-8", "9-16", "17-24", "25-31"])
def test_every_name_length(ctx, lengths):
    """pre_len % 8 of every value, both the `left > 4` and the `left <= 4` compare of parse_line_words, every key-word count of parse_line_flex."""
    fields = [(("n%02d_" % ln + "abcdefghijklmnopqrstuvwxyz0123456")[:ln], (I, S, L)[ln % 3]) for ln in lengths]
    assert [len(nm) for nm, _ in fields] == list(lengths)
    _three_writers(ctx, fields, n=300, seed=lengths[0])


def test_names_that_are_prefixes_or_differ_in_one_byte(ctx):
    names = ["a", "ab", "abc", "abcdefgh", "abcdefghi", "abcdefghij", "name_x", "name_y", "abcdefgh_1x", "abcdefgh_2x", "abcdefghijklmnopqrstuvwx1", "abcdefghijklmnopqrstuvwx2",
             "abcdefghijklmnopqrstuvwxyz01234", "abcdefghijklmnopqrstuvwxyz01235"]
    fields = [(nm, (I, L, S)[k % 3]) for k, nm in enumerate(names)]
    rows = _three_writers(ctx, fields, n=300, seed=3)
    # a key one byte off a schema name is a member that is not in the schema: the schema's own member is then missing
    for k, nm in enumerate(names):
        for other in (nm[:-1] + "!", nm + "x" if len(nm) < 31 else nm[:-1], "x" + nm[1:]):
            if other in names:
                continue
            for writer in range(3):
                bad = _write([(other if n2 == nm else n2, v) for n2, v in rows[k]], writer, k)
                text = _write(rows[0], writer, 0) + b"\n" + bad + b"\n"
                assert _agree(ctx, text, fields) == "missing"


@pytest.mark.parametrize("n_fields", [1, 4, 5, 8, 9, 16])
def test_field_counts_around_the_unrolled_instances(ctx, n_fields):
    fields = [("f%d" % k, (L, I, S, I)[k % 4]) for k in range(n_fields)]
    _three_writers(ctx, fields, seed=n_fields)


def test_limits_of_the_schema(ctx):
    from flock_amd import FlockGpuError, _ffi
    text = _dev_bytes(b'{"a":1}\n')
    for fields, code in (([("f%d" % k, I) for k in range(17)], _ffi.ERR_UNSUPPORTED), ([("n" * 32, I)], _ffi.ERR_UNSUPPORTED),
                         ([("", I)], _ffi.ERR_UNSUPPORTED)):           # (an empty name: refused with the too-long ones, as the code stands)
        with pytest.raises(FlockGpuError) as e:
            ctx.json_lines_decode(text, fields)
        assert e.value.code == code, str(e.value)
    got, n = ctx.json_lines_decode(_dev_bytes(b'{"%s":5}\n' % (b"n" * 31)), [("n" * 31, I)])
    assert n == 1 and got["n" * 31].cpu().tolist() == [5]
    spec, cols, rows = (_ffi.JsonField * 1)(_ffi.JsonField(b"a", _ffi.JSON_INT32)), (_ffi.JsonColumn * 1)(), C.c_int64(0)
    assert ctx._lib.flockgpu_json_lines_decode(ctx._h, text.data_ptr(), text.numel(), spec, 0, cols, C.byref(rows)) == _ffi.ERR_INVALID
    assert ctx._lib.flockgpu_json_lines_decode(ctx._h, text.data_ptr(), text.numel(), spec, 1, cols, C.byref(rows)) == _ffi.OK and rows.value == 1
    assert ctx._lib.flockgpu_abi_version() == 1


# ---- seams of the line index and of the stage -----------------------------------------------------------------------------------------------------------------------
def _fill(n):
    """n bytes (n >= 15) of short well-formed compact lines."""
    out = b'{"a":7,"b":"x"}\n' * ((n - 32) // 16 if n >= 48 else 0)
    rest = n - len(out)
    return out + b'{"a":7,"b":"' + b"y" * (rest - 15) + b'"}\n'


def _at(record, key, where):
    """A text in which byte `key` of `record` lies at offset `where`, with lines before and after it."""
    text = _fill(where - key) + record + b'{"a":8,"b":"after"}\n' * 3
    assert text[where] == record[key]
    return text


@pytest.mark.parametrize("where", [63, 64, 4095, 4096, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE])
def test_newline_at_a_seam(ctx, where):
    """A line's newline as the last byte of a lane's 64 bytes, of a wave's 4 KiB, of a tile -- and as the first byte of the next."""
    for rec in (b'{"a":5,"b":"seam"}\n', b'{"b": "se\\nam", "a": 5}\n'):
        _, n = _check(ctx, _at(rec, len(rec) - 1, where), AB)
        assert n >= 5


def test_cr_lf_split_across_a_tile_and_a_line_that_starts_one(ctx):
    rec = b'{"a":5,"b":"tail"}\r\n'
    _check(ctx, _at(rec, rec.index(b"\n"), TILE), AB)                          # '\r' | '\n'
    _check(ctx, _at(rec, rec.index(b"\n"), 2 * TILE), AB)
    _check(ctx, _at(rec, 0, TILE), AB)                                         # the line's first byte is the tile's first
    _check(ctx, _at(b'{"a": 5, "b": "first"}\n', 0, 2 * TILE), AB)


def test_a_line_longer_than_three_tiles_and_the_stage(ctx):
    big = b"line\\n" * 8400                                                     # escapes, no raw newline
    text = b'{"a":1,"b":"before"}\n' * 3 + b'{"a":2,"b":"' + big + b'"}\n' + b'{"a":3,"b":"after"}\n' * 3
    assert len(big) > 3 * TILE and len(big) > STAGE_MAX and not is_staged(text)
    got, n = _check(ctx, text, AB)
    assert n == 7 and got["a"].cpu().tolist() == [1, 1, 1, 2, 3, 3, 3] and got["b"].offsets.cpu().tolist()[4] - got["b"].offsets.cpu().tolist()[3] == 5 * 8400


def test_a_wave_without_a_newline(ctx):
    """Lanes 64..127 of the first tile (bytes 4096 .. 8191) see no newline at all; the waves on both sides do."""
    head = _fill(4096)
    text = head + b'{"a":2,"b":"' + b"w" * 5000 + b'"}\n' + _fill(3000)
    assert text[4095:4096] == b"\n" and b"\n" not in text[4096:8192] and b"\n" in text[8192:12288]
    _check(ctx, text, AB)


@pytest.mark.parametrize("n_lines", [1, 255, 256, 257, 512, 513])
def test_the_last_workgroup_holds_one_line(ctx, n_lines):
    lines = [b'{"a":%d,"b":"%s"}' % (k, b"z" * (k % 5)) for k in range(n_lines)]
    for writer_sep in (b",", b", "):
        text = b"\n".join(ln.replace(b",", writer_sep) for ln in lines)
        want = json_ref.decode(text, AB)
        _check(ctx, text + b"\n", AB, want)
        _check(ctx, text, AB, want)


@pytest.mark.parametrize("residue", [0, 1, 7, 15])
@pytest.mark.parametrize("writer", [0, 1])
def test_a_workgroup_that_just_fits_the_stage(ctx, residue, writer):
    """The second workgroup's 256 lines with b1 - a0 + 16 one below the stage, the stage exactly, one above it -- its first byte at `residue` mod 16: staged,
    staged, read from global memory, and the same rows each time."""
    def line(k, length):                                                        # `length` bytes with the newline
        head = (b'{"a":%d,"b":"' if writer == 0 else b'{"a": %d, "b": "') % k
        return head + b"s" * (length - len(head) - 3) + b'"}\n'
    first = b"".join(line(k, 180) for k in range(255)) + line(255, 180 + residue)           # 46080 + residue bytes: the next workgroup starts there
    assert len(first) % 16 == residue
    seen = []
    for delta in (-1, 0, 1):
        total = STAGE_MAX - 16 - residue + delta                                # the second workgroup's bytes: b1 - b0
        second = b"".join(line(256 + k, 192) for k in range(255)) + line(511, total - 255 * 192)
        text = first + second + line(512, 40)
        span, stage = block_span(text, 1)
        assert stage == STAGE_MAX and span == STAGE_MAX + delta
        seen.append(span <= stage)
        _check(ctx, text, AB)
    assert seen == [True, True, False]


# ---- the first offender among many lines ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("writer", ["compact", "python"])
def test_first_offender_among_many_lines(writer):
    """The line number over many workgroups, index tiles and both kernels: the FIRST bad line wins, whichever lane meets one first.  With Python's separators the
    context is on the `straight` route by then (the second kernel alone, every workgroup)."""
    from flock_amd import GpuContext
    fields = [("k", I), ("v", L)]
    fmt = b'{"k":%d,"v":%d}' if writer == "compact" else b'{"k": %d, "v": %d}'
    lines = [fmt % (i, i * 1003) for i in range(40_000)]
    # far apart -- other workgroups, other index tiles -- and of three kinds: INVALID (malformed, in a member that is not in the schema), UNSUPPORTED, out of range
    bad = {777: (b'{"k":1,"v":2,"z":[1}}', "malformed"), 20_001: ((fmt % (5, 6)).replace(b"6}", b"6.5}"), "number"), 39_000: (fmt % (2147483648, 1), "range")}
    for at, (line, _) in bad.items():
        lines[at] = line
    ctx = GpuContext(0)
    try:
        if writer == "python":
            small = b"\n".join(lines[:600]) + b"\n"
            for _ in range(3):                                                 # the first call sets the route, the next ones run on it
                _check(ctx, small, fields)
        for at in (777, 20_001, 39_000):
            text = b"\n".join(lines) + b"\n"
            assert len(text) < 1_150_000
            with pytest.raises(json_ref.JsonError) as r:
                json_ref.decode(text, fields)
            assert (r.value.line, r.value.code) == (at + 1, bad[at][1])
            assert _refusal(ctx, text, fields) == (r.value.status, at + 1, json_ref.MESSAGES[bad[at][1]])
            lines[at] = fmt % (0, 0)
        _check(ctx, b"\n".join(lines) + b"\n", fields)
    finally:
        ctx.close()


# ---- the route hint ---------------------------------------------------------------------------------------------------------------------------------------------------
def _writer_text(kind, n=2048, bad_at=None):
    """compact: no workgroup needs the second kernel; python: all do; mix: two of eight do."""
    lines = []
    for k in range(n):
        spaced = kind == "python" or (kind == "mix" and k // LINES in (2, 5))
        lines.append((b'{"a": %d, "b": "r%d"}' if spaced else b'{"a":%d,"b":"r%d"}') % (k - 1000, k))
    if bad_at is not None:
        lines[bad_at] = lines[bad_at].replace(b'"b"', b'"b" "b"')
    return b"\n".join(lines) + b"\n"


def test_forty_calls_that_change_the_writer():
    from flock_amd import GpuContext
    texts = {k: _writer_text(k) for k in ("compact", "python", "mix")}
    wants = {k: json_ref.decode(t, AB) for k, t in texts.items()}
    ctx = GpuContext(0)
    try:
        order = ["compact", "python", "mix"] * 4 + ["python"] * 5 + ["compact", "mix", "python", "python", "compact"] * 4 + ["mix", "python", "compact"]
        assert len(order) == 40
        for kind in order:
            _check(ctx, texts[kind], AB, wants[kind])
    finally:
        ctx.close()


@pytest.mark.parametrize("with_errors", [False, True])
def test_a_run_of_one_writer_through_the_sixteenth_calls(with_errors):
    """34 calls of Python-separator text on a fresh context: call 1 finds the route, calls 2 .. 16 and 18 .. 32 run the second kernel alone, calls 17 and 33 try
    the compact walk first again.  The route is not visible from outside: what is asserted is every call's rows -- and, in the second run, the line of
    the error that calls 1, 2, 16, 17, 32 and 33 hold."""
    from flock_amd import GpuContext
    good = _writer_text("python", 700)
    want = json_ref.decode(good, AB)
    bad = _writer_text("python", 700, bad_at=555)
    ctx = GpuContext(0)
    try:
        for call in range(1, 35):
            if with_errors and call in (1, 2, 16, 17, 32, 33):
                assert _refusal(ctx, bad, AB) == ("invalid", 556, json_ref.MESSAGES["malformed"]), call
            else:
                _check(ctx, good, AB, want)
    finally:
        ctx.close()


# ---- the text at the end of its buffer ------------------------------------------------------------------------------------------------------------------------------------
def _ending(kind, ending, total):
    """`total` bytes of lines of one writer that end WITHOUT a newline: in '}', in a digit (the object is not closed: an error), or in '"' (likewise)."""
    unit = {"compact": b'{"a":7,"b":"u"}\n', "python": b'{"a": 7, "b": "u"}\n', "general": b'{"a":7,"z":[1],"b":"u"}\n'}[kind]
    sp = b" " if kind == "python" else b""
    z = b'"z":[1],' if kind == "general" else b""
    last = {"}": b'{%s"a":%s7,%s"b":%s"%%s"}' % (z, sp, sp, sp), "digit": b'{%s"b":%s"%%s",%s"a":%s7' % (z, sp, sp, sp), '"': b'{%s"a":%s7,%s"b":%s"%%s"' % (z, sp, sp, sp)}[ending]
    fill = unit * max(0, (total - len(last % b"") - 8) // len(unit))
    text = fill + last % (b"e" * (total - len(fill) - len(last % b"")))
    assert len(text) == total and not text.endswith(b"\n")
    return text


@pytest.mark.parametrize("length", range(1, 34))
def test_text_ends_at_the_end_of_its_buffer(ctx, length):
    """Lengths of 1 .. 33 bytes beyond a multiple of 16, short and beyond one index tile: the last partial 16-byte chunk is the stage's byte-wise copy and the
    walkers' last reads (under FLOCK_TEST_GUARDED=1 the text ends where mapped memory ends, and a read past it faults).  A cut that the reference refuses
    is compared on status and line like any other."""
    for base in (48, TILE + 48):
        for kind in ("compact", "python", "general"):
            for ending, code in (("}", None), ("digit", "malformed"), ('"', "malformed")):
                assert _agree(ctx, _ending(kind, ending, base + length), AB, at_end=True) == code


# ---- seeded one-byte mutants ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("part", range(4))
def test_mutants(ctx, seed, part):
    """Every mutant of the seed, each as line 3 of five in a call of its own: the reference's status and line, or its rows."""
    lines = mutants(seed)[part * 500:(part + 1) * 500]
    assert len(lines) == 500
    codes = [_agree(ctx, mutant_text(ln), MUTANT_FIELDS) for ln in lines]
    assert sum(c is None for c in codes) >= 100 and sum(c is not None for c in codes) >= 200
