"""tests/json_nullable_ref.py, the reference of flockgpu_json_lines_decode_nullable (json.hip A-JSONN1..7), held against Python itself, and the corpora
that tests/test_gpu_json_nullable.py decodes on the device:
  - every line of a seeded corpus (six types x {value, null, absent}, three writers) against json.loads: an accepted line agrees member for member, a
    None or a missing key there is a NULL here; an INVALID line is one json.loads rejects or one whose member has the wrong type or range;
  - every accepted Float64 equals float(text) BIT FOR BIT, and every number declined as UNSUPPORTED is one float(text) still parses;
  - hand-worked rows: repeated keys, {}, the near-null spellings, the number edges;
  - the one-byte mutants of texts with nulls and absent members: the mix of outcomes (each at least a fifth) is asserted here, on the reference alone."""
import json
import re
import struct

import numpy as np
import pytest

import json_nullable_ref as ref
from json_ref import _Bad
from test_json_reference import _refuse

I, L, U, D, T, S = "int32", "int64", "uint64", "float64", "timestamp_ms", "utf8"
FIELDS = [("i32", I), ("i64", L), ("u64", U), ("f64", D), ("ts", T), ("str", S)]           # every field nullable
ABSENT = object()                                                                         # a member that the line does not hold
RANGES = {I: (-(1 << 31), (1 << 31) - 1), L: (-(1 << 63), (1 << 63) - 1), T: (-(1 << 63), (1 << 63) - 1), U: (0, (1 << 64) - 1)}


def bits(v):
    return struct.pack("<d", v)


class Pairs(list):
    """An object as json.loads met it: its (key, value) pairs in order, repeated keys kept."""


def _texts(o):
    if isinstance(o, str):
        yield o
    elif isinstance(o, Pairs):
        for k, v in o:
            yield k
            yield from _texts(v)
    elif isinstance(o, list):
        for v in o:
            yield from _texts(v)


# ---- json.loads as the judge of one line ------------------------------------------------------------------------------------------------------------------------
def judge(line, fields):
    """{name: int | float | bytes | None} as json.loads reads the line under the schema (numbers through their own text: int(text), float(text); objects as
    their pairs, so that every occurrence of a repeated key is seen), or "refused" where it, or the schema, refuses the line."""
    errors = "strict"
    try:
        s = line.decode("utf-8")
    except UnicodeDecodeError:
        assert not re.search(rb"\\u[dD][cC][89a-fA-F]", line), "the judge cannot tell this escape from a raw byte"
        errors = "surrogateescape"
        s = line.decode("utf-8", errors)
    try:
        o = json.loads(s, parse_constant=_refuse, parse_int=lambda t: ("int", t), parse_float=lambda t: ("float", t), object_pairs_hook=Pairs)
        for v in _texts(o):
            v.encode("utf-8", errors)
    except (ValueError, RecursionError):
        return "refused"
    if not isinstance(o, Pairs):
        return "refused"
    row = {}
    for name, t, nullable in ref.normalise(fields):
        row[name] = None
        if not nullable and not any(k == name for k, _ in o):
            return "refused"
        for v in (v for k, v in o if k == name):        # every occurrence is checked and typed; the last one is the value
            if v is None:
                if not nullable:
                    return "refused"
                row[name] = None
            elif t == S:
                if not isinstance(v, str):
                    return "refused"
                row[name] = v.encode("utf-8", errors)
            elif not isinstance(v, tuple):              # true, a string, a container
                return "refused"
            elif t == D:
                row[name] = float(v[1])
            else:
                lo, hi = RANGES[t]
                if v[0] != "int" or not lo <= int(v[1]) <= hi or (t == U and v[1].startswith("-")):
                    return "refused"
                row[name] = int(v[1])
    return row


def same_row(got, want):
    return got.keys() == want.keys() and all(type(got[k]) is type(want[k]) and (bits(got[k]) == bits(want[k]) if isinstance(got[k], float) else got[k] == want[k])
                                             for k in got)


def check_line(line, fields):
    """The reference and the judge on one line -> the reference's row, or its error code."""
    want = judge(line, fields)
    try:
        got = ref.parse_line(line, fields)
    except _Bad as e:
        if e.args[0] not in ("key_escape", "depth", "float"):   # well-formed JSON that the decoder declines (a declined Float64: test_float64_tokens)
            assert want == "refused", (line, e.args, want)
        return e.args[0]
    assert want != "refused" and same_row(got, want), (line, got, want)
    return got


# ---- writers ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _value(v, escapes=False):
    if v is None:
        return b"null"
    if isinstance(v, bytes) and v[:1] == b"#":          # a number's own text
        return v[1:]
    if isinstance(v, int):
        return b"%d" % v
    return json.dumps(v, ensure_ascii=escapes).encode("utf-8", "surrogateescape")


def write(items, writer, k=0):
    """One line of (name, value) members: value an int, a str, b"#" + a number's text, None (null) or ABSENT.  writer 0: compact, the encoder's shape;
    1: a space after ':' and ',' with the members rotated; 2: strings with \\u escapes and a nested member that is not in the schema."""
    items = [(n, v) for n, v in items if v is not ABSENT]
    if writer == 1:
        r = k % max(len(items), 1)
        items = items[r:] + items[:r]
        return b"{" + b", ".join(b'"%s": %s' % (n.encode(), _value(v)) for n, v in items) + b"}"
    body = [b'"%s":%s' % (n.encode(), _value(v, writer == 2)) for n, v in items]
    if writer == 2:
        body.insert(k % (len(body) + 1), b'"not in the schema":[%d,{"k":"}","n":null}]' % k)
    return b"{" + b",".join(body) + b"}"


WORDS = ["", "plain", "two words, a comma", "q\"uote", "back\\slash", "tab\there", "café", "漢字", "\U0001F600", "{[:]}", "null", "nul\x01l", "\x7f\x1f"]
EXACT_FLOATS = [b"0", b"-0.0", b"3", b"0.1", b"1e22", b"1E-22", b"9007199254740992", b"123456.789e3", b"-2.5", b"1.50", b"100e-2", b"0e99", b"12345678901234.5"]


def float_token(rng):
    """A well-formed JSON number: 1 .. 18 digits, a fraction and an exponent now and then; about half of them inside the exact range."""
    whole = str(int(rng.integers(0, 10 ** int(rng.integers(1, 18)))))
    frac = "." + "".join(str(int(d)) for d in rng.integers(0, 10, int(rng.integers(1, 7)))) if rng.integers(0, 2) else ""
    exp = "eE"[int(rng.integers(0, 2))] + ["", "+", "-"][int(rng.integers(0, 3))] + str(int(rng.integers(0, 30))) if rng.integers(0, 3) == 0 else ""
    return ("-" if rng.integers(0, 4) == 0 else "").encode() + (whole + frac + exp).encode()


def a_value(rng, t, k):
    if t == S:
        return WORDS[int(rng.integers(0, len(WORDS)))] + WORDS[k % len(WORDS)]
    if t == D:
        while True:
            tok = EXACT_FLOATS[k % len(EXACT_FLOATS)] if k % 3 == 0 else float_token(rng)
            if ref.exact_f64(tok) is not None:
                return b"#" + tok
            k += 3
    lo, hi = RANGES[t]
    edge = [lo, hi, 0, -1 if lo else 1, hi // 2 + 1][k % 5]
    return edge if k % 4 == 0 else int(rng.integers(max(lo, -10 ** int(rng.integers(1, 19))), min(hi, 10 ** int(rng.integers(1, 19))), dtype=np.int64))


def corpus(seed, count, fields=FIELDS, p_null=0.2, p_absent=0.1, writers=(0, 1, 2)):
    """`count` well-formed lines over `fields`: each member a value, null or absent."""
    rng = np.random.default_rng(9100 + seed)
    out = []
    for k in range(count):
        items = []
        for name, t, nullable in ref.normalise(fields):
            u = rng.random()
            items.append((name, None if nullable and u < p_null else ABSENT if nullable and u < p_null + p_absent else a_value(rng, t, k + len(items))))
        out.append(write(items, writers[k % len(writers)], k))
    return out


# ---- the corpus against json.loads ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_corpus_lines_agree_with_json_loads(seed):
    lines = corpus(seed, 600)
    states = {"null": 0, "absent": 0, "value": 0}
    for line in lines:
        row = check_line(line, FIELDS)
        assert isinstance(row, dict), (line, row)
        o = json.loads(line.decode("utf-8", "surrogateescape"))
        for name, _ in FIELDS:
            states["absent" if name not in o else "null" if o[name] is None else "value"] += 1
            assert (row[name] is None) == (o.get(name) is None)
    assert min(states.values()) > 200
    cols, valid, nulls = ref.decode(b"\n".join(lines) + b"\n", FIELDS)
    for name, t in FIELDS:
        assert nulls[name] == int((valid[name] == 0).sum()) > 0
        zero = cols[name].offsets[1:] - cols[name].offsets[:-1] if t == S else cols[name]
        assert not np.any(zero[valid[name] == 0])      # a NULL is value 0 / length 0


def test_float64_tokens():
    """Bit for bit against float(text) inside the exact range; outside it the text is still a number float() parses."""
    rng = np.random.default_rng(9200)
    tokens = EXACT_FLOATS + [float_token(rng) for _ in range(4000)] + [b"9007199254740993", b"1e23", b"1e-23", b"0.30000000000000004", b"1e400", b"123456789012345678901234567890"]
    inside = 0
    for tok in tokens:
        v = ref.exact_f64(tok)
        if v is None:
            float(tok)
            with pytest.raises(_Bad) as e:
                ref.parse_line(b'{"f64":' + tok + b"}", FIELDS)
            assert e.value.args == ("float", "f64"), tok
        else:
            inside += 1
            assert bits(v) == bits(float(tok)), tok
            assert bits(ref.parse_line(b'{"f64": ' + tok + b" }", FIELDS)["f64"]) == bits(float(tok))
    assert len(tokens) // 5 < inside < len(tokens) * 4 // 5
    assert bits(ref.exact_f64(b"-0.0")) == bits(-0.0) != bits(0.0) and ref.exact_f64(b"3") == 3.0
    assert ref.exact_f64(b"9007199254740992") == 2.0 ** 53 and ref.exact_f64(b"90071992547409920e-1") == 2.0 ** 53
    assert ref.exact_f64(b"1000000000000000000000") == 1e21 and ref.exact_f64(b"1e22") == 1e22 and ref.exact_f64(b"10e22") is None


# ---- hand-worked lines --------------------------------------------------------------------------------------------------------------------------------------------------
AB = [("a", L), ("b", S)]
AB_REQ = [("a", L, False), ("b", S)]
HAND = [
    (b'{"a":1,"b":"x"}', AB, {"a": 1, "b": b"x"}),
    (b'{"a":null,"b":null}', AB, {"a": None, "b": None}),
    (b"{}", AB, {"a": None, "b": None}),
    (b" { } \r", AB, {"a": None, "b": None}),
    (b"{}", AB_REQ, "missing"),
    (b'{"b":"x"}', AB_REQ, "missing"),
    (b'{"a":null,"b":"x"}', AB_REQ, "malformed"),            # a required field keeps the first entry point's answer to null
    (b'{"a":7}', AB_REQ, {"a": 7, "b": None}),
    (b'{"b":""}', AB, {"a": None, "b": b""}),                # "" is a value
    (b'{"a":1,"a":null,"b":"x"}', AB, {"a": None, "b": b"x"}),   # the last occurrence wins
    (b'{"a":null,"a":1,"b":"x"}', AB, {"a": 1, "b": b"x"}),
    (b'{"a":1,"a":true,"b":"x"}', AB, "malformed"),          # every occurrence is checked and typed
    (b'{"a":1.5,"a":null}', AB, "number"),
    (b'{"b":"x","b":null,"b":"y\\n"}', AB, {"a": None, "b": b"y\n"}),
    (b'{"a":nul}', AB, "malformed"),
    (b'{"a":NULL}', AB, "malformed"),
    (b'{"a":nullx}', AB, "malformed"),
    (b'{"a":null x}', AB, "malformed"),
    (b'{"a": null ,"zz":null}', AB, {"a": None, "b": None}),
    (b'{"a":true}', AB, "malformed"),
    (b'{"a":"1"}', AB, "malformed"),
    (b'{"b":1}', AB, "malformed"),
    (b"", AB, "blank"),
    (b"null", AB, "malformed"),
    (b'{"t":"2020-01-01 00:00:00"}', [("t", T)], "malformed"),   # a timestamp is its integer
    (b'{"t":-9223372036854775808}', [("t", T)], {"t": -(1 << 63)}),
    (b'{"t":9223372036854775808}', [("t", T)], "range"),
    (b'{"u":18446744073709551615}', [("u", U)], {"u": (1 << 64) - 1}),
    (b'{"u":9223372036854775808}', [("u", U)], {"u": 1 << 63}),
    (b'{"u":18446744073709551616}', [("u", U)], "range"),
    (b'{"u":100000000000000000000}', [("u", U)], "range"),
    (b'{"u":-0}', [("u", U)], "range"),
    (b'{"u":-1}', [("u", U)], "range"),
    (b'{"u":1e3}', [("u", U)], "number"),
    (b'{"u":01}', [("u", U)], "malformed"),
    (b'{"d":3}', [("d", D)], {"d": 3.0}),
    (b'{"d":-0.0}', [("d", D)], {"d": -0.0}),
    (b'{"d":123456.789e3}', [("d", D)], {"d": 123456789.0}),
    (b'{"d":1e23}', [("d", D)], "float"),
    (b'{"d":9007199254740993}', [("d", D)], "float"),
    (b'{"d":1e23x}', [("d", D)], "malformed"),               # the grammar, what follows the number, then the range
    (b'{"d":+1}', [("d", D)], "malformed"),
    (b'{"d":01}', [("d", D)], "malformed"),
    (b'{"d":.5}', [("d", D)], "malformed"),
    (b'{"d":1.}', [("d", D)], "malformed"),
    (b'{"d":1e}', [("d", D)], "malformed"),
    (b'{"d":nan}', [("d", D)], "malformed"),
    (b'{"d":NaN}', [("d", D)], "malformed"),
    (b'{"d":Infinity}', [("d", D)], "malformed"),
    (b'{"d":-Infinity}', [("d", D)], "malformed"),
    (b'{"d":"1.5"}', [("d", D)], "malformed"),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_worked_lines(case):
    line, fields, want = HAND[case]
    got = check_line(line, fields)
    assert same_row(got, want) if isinstance(want, dict) else got == want, (line, got)


def test_decode_columns_and_the_first_offender():
    text = b'{"a":1,"b":"x"}\n{}\n{"b":""}\n{"a":null,"b":"yz"}'
    cols, valid, nulls = ref.decode(text, AB)
    assert cols["a"].tolist() == [1, 0, 0, 0] and valid["a"].tolist() == [1, 0, 0, 0] and nulls == {"a": 3, "b": 1}
    assert cols["b"].offsets.tolist() == [0, 1, 1, 1, 3] and valid["b"].tolist() == [1, 0, 1, 1] and bytes(cols["b"].data) == b"xyz"
    cols, valid, nulls = ref.decode(b'{"a":1}\n', AB_REQ)
    assert "a" not in valid and valid["b"].tolist() == [0] and nulls == {"a": 0, "b": 1}
    with pytest.raises(ref.JsonError) as e:
        ref.decode(b'{"d":1}\n{"d":1e23}\n{"d":}\n', [("d", D)])
    assert (e.value.line, e.value.status, e.value.message) == (2, "unsupported", ref.MESSAGES["float"] % "d")
    with pytest.raises(ref.JsonError) as e:
        ref.decode(b'{"d":1}\n{"d":}\n{"d":1e23}\n', [("d", D)])
    assert (e.value.line, e.value.status, e.value.message) == (2, "invalid", ref.MESSAGES["malformed"])
    assert ref.decode(b"", AB)[0]["a"].tolist() == []


# ---- the seeded one-byte mutants --------------------------------------------------------------------------------------------------------------------------------------
MUTANT_FIELDS = FIELDS[:3] + [("f64", D), ("ts", T, False), ("str", S)]     # one required field among the nullable ones
MUTANT_GOOD = b'{"i32":1,"i64":null,"u64":2,"f64":0.5,"ts":3,"str":"good"}'
ALPHABET = b'{}[]":,\\ 0123456789e.-tnulNE+\t\xc3'


def mutants(seed, count):
    """`count` lines, each ONE byte (deleted, inserted or replaced) away from a well-formed line of the corpus -- nulls and absent members included, all
    three writers."""
    rng = np.random.default_rng(9300 + seed)
    good = corpus(50 + seed, count, MUTANT_FIELDS, p_null=0.25, p_absent=0.15)
    out, k = [], 0
    while len(out) < count:
        line = bytearray(good[k % len(good)])
        k += 1
        at, op, c = int(rng.integers(0, len(line))), int(rng.integers(0, 3)), ALPHABET[int(rng.integers(0, len(ALPHABET)))]
        if op == 0:
            del line[at]
        elif op == 1:
            line.insert(at, c)
        elif line[at] == c:
            continue
        else:
            line[at] = c
        if b"\n" not in line:
            out.append(bytes(line))
    return out


def mutant_text(line):
    """The mutant as line 3 of five."""
    return b"\n".join([MUTANT_GOOD, MUTANT_GOOD, line, MUTANT_GOOD, MUTANT_GOOD]) + b"\n"


MUTANT_RUNS = [(0, 700), (1, 700)]            # (seed, count): the corpora tests/test_gpu_json_nullable.py decodes on the device, and the ones judged here


@pytest.mark.parametrize("seed,count", MUTANT_RUNS)
def test_mutants(seed, count):
    """The reference against json.loads on every mutant, and the mix of outcomes that makes the device differential worth running: accepted and refused
    mutants are each at least a fifth of the corpus -- asserted for exactly the corpora the device sees."""
    lines = mutants(seed, count)
    outcomes = [check_line(line, MUTANT_FIELDS) for line in lines]
    accepted = sum(isinstance(o, dict) for o in outcomes)
    assert accepted * 5 >= len(lines) and (len(lines) - accepted) * 5 >= len(lines), (accepted, len(lines))
    assert {"malformed", "missing", "number", "range"} <= {o for o in outcomes if not isinstance(o, dict)}
    assert any(isinstance(o, dict) and None in o.values() for o in outcomes)
