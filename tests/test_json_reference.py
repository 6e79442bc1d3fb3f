"""tests/json_ref.py, the reference the GPU tests compare flockgpu_json_lines_decode with (json.hip A-JSON1..9), checked on the CPU against Python's
json.loads LINE BY LINE: hand-worked lines, the three generated NEXMark relations, the ERRORS list and the well-formed edge texts that
tests/test_gpu_json_edges.py runs on the device, and the seeded one-byte mutants of its differential.  Accept / reject and the values must agree.

Where json.loads and the reference differ ON PURPOSE (`judge` closes the first four, so that they agree after all; `check_line` lets the last three pass):
  * NaN / Infinity / -Infinity: json.loads takes them; `parse_constant` refuses them here;
  * a lone surrogate escape: json.loads returns a str that cannot be encoded; the judge refuses a line whose strings do not encode;
  * integers beyond 64 (or 32) bits: json.loads returns a big int; the judge applies the column's range;
  * a fraction or an exponent in a schema integer: json.loads returns a float; the judge takes only `int` (the reference says UNSUPPORTED, both refuse);
  * invalid UTF-8: json.loads refuses the bytes, the reference copies them (A-JSON7); the judge decodes such a line with surrogateescape, which hands
    the bytes through;
  * an escape in a key of the line's object (UNSUPPORTED, A-JSON6): json.loads resolves it;
  * brackets more than 64 deep in a dropped member (UNSUPPORTED, A-JSON6): json.loads follows them;
  * a repeated key whose EARLIER occurrence is malformed for its column: json.loads keeps only the last, the reference types every occurrence (A-JSON3).
    No generated line holds one (the mutants' names are more than one edit apart); hand-worked below."""
import json
import re

import numpy as np
import pytest

import json_ref
import oracle
from json_ref import JsonError, decode, parse_line
from test_oracle_json import SCHEMAS, _events

I, L, S = "int32", "int64", "utf8"
AB = [("a", I), ("b", S)]
AL = [("a", L), ("b", S)]
GOOD = b'{"a":1,"b":"x"}'


# ---- json.loads as the judge of one line ------------------------------------------------------------------------------------------------------------------------
def _refuse(name):
    raise ValueError(name)


def _strings(o):
    if isinstance(o, str):
        yield o
    elif isinstance(o, list):
        for v in o:
            yield from _strings(v)
    elif isinstance(o, dict):
        for k, v in o.items():
            yield k
            yield from _strings(v)


def judge(line, fields):
    """{name: int | bytes} as json.loads reads the line under the schema, or None where it (or the schema) refuses the line."""
    errors = "strict"
    try:
        s = line.decode("utf-8")
    except UnicodeDecodeError:
        assert not re.search(rb"\\u[dD][cC][89a-fA-F]", line), "the judge cannot tell this escape from a raw byte"
        errors = "surrogateescape"
        s = line.decode("utf-8", errors)
    try:
        o = json.loads(s, parse_constant=_refuse)
        for v in _strings(o):
            v.encode("utf-8", errors)
    except (ValueError, RecursionError):         # (UnicodeEncodeError is a ValueError)
        return None
    if not isinstance(o, dict):
        return None
    row = {}
    for name, t in fields:
        v = o.get(name)
        if t == S:
            if not isinstance(v, str):
                return None
            row[name] = v.encode("utf-8", errors)
        else:
            bits = 32 if t == I else 64
            if type(v) is not int or not -(1 << bits - 1) <= v < (1 << bits - 1):
                return None
            row[name] = v
    return row


def check_line(line, fields):
    """The reference and the judge on one line -> the reference's row, or its error code."""
    want = judge(line, fields)
    try:
        got = parse_line(line, fields)
    except json_ref._Bad as e:
        if e.args[0] not in ("key_escape", "depth"):
            assert want is None, (line, e.args[0], want)
        return e.args[0]
    assert got == want, (line, got, want)
    return got


# ---- the texts tests/test_gpu_json_edges.py decodes on the device ---------------------------------------------------------------------------------------------------
def _err(bad, code, fields=AB, good=GOOD, at=3):
    """The bad line as line `at` (never 1) among good ones."""
    lines = [good] * 4
    lines.insert(at - 1, bad)
    return (b"\n".join(lines) + b"\n", fields, (json_ref.STATUS[code], at, code))


def _errors():
    out = []
    add = lambda *a, **k: out.append(_err(*a, at=2 + len(out) % 4, **k))
    # structure
    for bad, code in ((b'{"a":2}', "missing"), (b"{}", "missing"), (b"{ }", "missing"), (b'{"b":"y","z":2}', "missing"), (b'{"a":2,"b":"y"', "malformed"),
                      (b'{"a":2,"b":"y",}', "malformed"), (b'{"a":2,"b":"y"} x', "malformed"), (b'{"a":2,"b":"y"}}', "malformed"), (b'{"a":2,"b":"y"},', "malformed"),
                      (b'{"a" 2,"b":"y"}', "malformed"), (b'{"a":2 "b":"y"}', "malformed"), (b'{"a":2,,"b":"y"}', "malformed"), (b'{,"a":2,"b":"y"}', "malformed"),
                      (b'{a:2,"b":"y"}', "malformed"), (b"[1]", "malformed"), (b"1", "malformed"), (b'"x"', "malformed"), (b'[{"a":2,"b":"y"}]', "malformed"),
                      (b'{"a":2,"b":"y"', "malformed"), (b"{", "malformed"), (b'{"a"', "malformed"), (b'{"a":', "malformed"), (b'{"a":2,', "malformed")):
        add(bad, code)
    # schema integers, as Int32 and as Int64, as the compact writer and as Python's put them
    for fields in (AB, AL):
        for v, code in ((b"-", "malformed"), (b"+1", "malformed"), (b"01", "malformed"), (b"-01", "malformed"), (b"1x", "malformed"), (b"1]", "malformed"),
                        (b"1.", "malformed"), (b"1e", "malformed"), (b"1.e3", "malformed"), (b"1e+", "malformed"), (b"1.5x", "malformed"), (b".5", "malformed"),
                        (b"1.5", "number"), (b"1e3", "number"), (b"1E+2", "number"), (b"-0.0", "number"), (b"12.5e-7", "number"),
                        (b'"1"', "malformed"), (b"true", "malformed"), (b"null", "malformed"), (b"[1]", "malformed"), (b"", "malformed"),
                        (b"12345678901234567890", "range"), (b"-12345678901234567890", "range"), (b"123456789012345678901234567890", "range"),
                        (b"12345678901234567890.5", "number"), (b"12345678901234567890x", "malformed")):
            add(b'{"a":%s,"b":"y"}' % v, code, fields=fields)
            add(b'{"b": "y", "a": %s}' % v, code, fields=fields)
    for v in (b"2147483648", b"-2147483649", b"9223372036854775807"):
        add(b'{"a":%s,"b":"y"}' % v, "range")
        add(b'{"a": %s, "b": "y"}' % v, "range")
    for v in (b"9223372036854775808", b"-9223372036854775809", b"18446744073709551616"):
        add(b'{"a":%s,"b":"y"}' % v, "range", fields=AL)
        add(b'{"a": %s, "b": "y"}' % v, "range", fields=AL)
    add(b'{"a":1,"b":5}', "malformed")                  # a number where a string is due
    add(b'{"a":1,"b":null}', "malformed")
    add(b'{"a":1,"b":["y"]}', "malformed")
    # strings
    for v in (b'y\x01z', b'y\tz', b'\x1f', b'y\\qz', b'\\u12', b'\\u12G4', b'\\u 123', b'\\ud800x', b'\\ud800\\ud800', b'\\ud800\\n', b'\\uD800\\u0041',
              b'\\udc00', b'\\uDFFF', b'\\ud83d', b'\\ud83d\\ude', b'\\ud83d\\', b'\\U0041', b"\\'"):
        add(b'{"a":1,"b":"%s"}' % v, "malformed")
        add(b'{"b": "%s", "a": 1}' % v, "malformed")
    add(b'{"a":1,"b":"y\\', "malformed")                 # a backslash as the line's last byte
    add(b'{"a":1,"b":"y\\"}', "malformed")               # ... and one that takes the closing quote
    add(b'{"a":1,"b":"y}', "malformed")
    # members that are not in the schema
    for v in (b"xyz", b"tru", b"nulll", b"True", b"falsey", b"nul", b"1.2.3", b"-", b"01", b"-01", b"1.", b".5", b"1e", b"1e+", b"+1", b"0x10", b"NaN", b"-Infinity",
              b"[1}", b'{"a":1]', b'{"a" 1}', b'{"a":}', b"{1:2}", b'{"a"}', b'{"a":1,}', b'{,"a":1}', b'{"a":1 "b":2}', b'{"a":1,"b"}', b"{[]}", b'{"a":1:2}',
              b"[,]", b"[1,]", b"[,1]", b"[1 2]", b"[1,,2]", b'[1:2]', b'["a":1]', b"[[1,2]}", b'{"k":[1,2}}', b"[1,2", b'{"k":[1,2]', b"[", b"{", b'["abc]', b'{"k":"abc}',
              b'["\\q"]', b'["\\ud800"]', b'{"\\ud800":1}', b'["\x01"]', b"[tru]", b"[1.]", b"[01]", b'{"k":xyz}', b"", b"]", b"}"):
        add(b'{"a":1,"b":"y","z":%s}' % v, "malformed")
        add(b'{"z": %s, "a": 1, "b": "y"}' % v, "malformed")
    add(b'{"a":1,"b":"y","z":' + b"[" * 65 + b"]" * 65 + b"}", "depth")
    add(b'{"a":1,"z":' + b'{"k":' * 64 + b"[1]" + b"}" * 64 + b',"b":"y"}', "depth")
    add(b'{"a":1,"b":"y","z":' + b"[" * 65 + b"}", "depth")            # reported where the 65th bracket opens, whatever follows it
    # blank lines
    out.append((GOOD + b"\n\n" + GOOD + b"\n", AB, ("unsupported", 2, "blank")))
    out.append((GOOD + b"\n" + GOOD + b"\n\n", AB, ("unsupported", 3, "blank")))
    out.append((GOOD + b"\n" + GOOD + b"\n\r\n" + GOOD + b"\n", AB, ("unsupported", 3, "blank")))
    out.append((GOOD + b"\n" + GOOD + b"\n \t\r", AB, ("unsupported", 3, "blank")))   # white space after the last newline
    out.append((GOOD + b"\n" + GOOD + b"\n ", AB, ("unsupported", 3, "blank")))
    # an escape in a key: a schema name or not
    add(b'{"\\u0061":2,"b":"y"}', "key_escape")
    add(b'{"a":2,"b":"y","z\\n":1}', "key_escape")
    add(b'{"a": 2, "\\u0062": "y"}', "key_escape")
    add(b'{"a":2,"b":"y","z\\q":1}', "malformed")         # (a malformed escape in a key is malformed)
    return out


ERRORS = _errors()


def _nested(levels, leaf=b"1"):
    """`levels` brackets deep, objects and arrays taking turns."""
    v = leaf
    for k in range(levels):
        v = b'{"k":' + v + b"}" if k % 2 else b"[" + v + b"]"
    return v


def _well_formed():
    """[(what, text, fields)]: the well-formed edges.  Every line decodes; the expected columns are the reference's."""
    out = []
    lines = []
    for cp in ("0000", "007f", "0080", "07ff", "0800", "d7ff", "e000", "ffff", "d800\\udc00", "dbff\\udfff", "d83d\\ude00", "00e9", "000a", "0022", "005c"):
        for esc in (cp, cp.upper().replace("\\U", "\\u")):
            lines += [b'{"a":%d,"b":"\\u%s"}' % (len(lines), esc.encode()), b'{"a":%d,"b":"pre\\u%spost"}' % (len(lines), esc.encode()),
                      b'{"b": "\\u%s\\u%s", "a": %d}' % (esc.encode(), esc.encode(), len(lines))]
    out.append(("u_escapes", lines, AB))
    singles = [b'\\"', b"\\\\", b"\\/", b"\\b", b"\\f", b"\\n", b"\\r", b"\\t"]
    lines = [b'{"a":%d,"b":"%s%s"}' % (i * 8 + j, x, y) for i, x in enumerate(singles) for j, y in enumerate(singles)]
    lines += [b'{"a":1,"b":"%s"}' % x for x in singles] + [b'{"a":2,"b":"%s"}' % b"".join(singles), b'{"a":3,"b":"\\nabc\\t"}', b'{"a":4,"b":"abc\\\\"}',
                                                         b'{"a":5,"b":"abc\\"def"}', b'{"a":6,"b":"\\\\\\"\\\\"}', b'{"a":7,"b":"a\\/b/c"}']
    for k in range(1, 10):                                 # k backslashes before a quote: an odd run takes the quote, and the value goes on to the next one
        lines.append(b'{"a":%d,"b":"x%s"%s}' % (k, b"\\" * k, b'"' if k % 2 else b""))
        lines.append(b'{"b": "x%s"%s, "a": %d}' % (b"\\" * k, b'"' if k % 2 else b"", k))
    out.append(("escape_placement", lines, AB))
    out.append(("repeated_keys", [b'{"a":1,"b":"e\\n","b":"plain"}', b'{"a":2,"b":"plain","b":"e\\n"}', b'{"a":3,"b":"x","a":7}', b'{"a": 4, "b": "x", "a": 8}',
                                  b'{"a":5,"z":1,"b":"x","a":9,"z":2}', b'{"a":6,"b":"first","a":-6,"b":"","a":10}', b'{"a":1,"b":"x","z":{"k":1,"k":2}}',
                                  b'{"a":11,"b":"\\u00e9","b":"\xc3\xa9"}', b'{"a":2147483647,"b":"x","a":-2147483648}'], AB))
    shapes = [b"null", b"true", b"false", b"0", b"-0", b"7", b"1.5", b"-1e-3", b"1E+2", b"0.0e0", b"-0.5E-05", b"123456789012345678901234567890", b"1e999", b'""', b'"s"',
              b"[]", b"{}", b"[ ]", b"{ }", b"[[]]", b"[{}]", b'{"k":[]}', b'{"k":{"k":{}}}', b'[1,"a",null,[true,false],{"x":1.5}]', b'"}]\\"\\\\"', b'{"}":"]","\\"":"\\\\"}',
              b'["[","{",",",":"]', b"[ 1 , 2 ]", b'{ "k" : 1 , "l" : [ ] }', b'{"k\\n":1,"k\\n":2,"":3}', b"[\t1\t,\r2 ]", b'"\\ud83d\\ude00"', b'["\xc3\xa9\xff"]',
              _nested(64), _nested(63, b"{}"), b"[" * 64 + b"]" * 64, b'{"k":' * 64 + b"null" + b"}" * 64, _nested(64, b'"]}"'), _nested(32) + b"", b"[" + _nested(63) + b"," + _nested(63) + b"]"]
    lines = []
    for i, v in enumerate(shapes):
        lines += [b'{"z":%s,"a":%d,"b":"x"}' % (v, i), b'{"a":%d,"z":%s,"b":"x"}' % (i, v), b'{"a":%d,"b":"x","z":%s}' % (i, v), b'{"a": %d, "y": %s , "b": "x", "z" :%s}' % (i, v, v)]
    out.append(("unknown_members", lines, AB))
    # -0 and the extremes of both types through the three walkers: compact text, a space after ':', an unknown member
    # (a text of ONE writer each: a workgroup that holds a line of another writer goes to the second kernel with all its lines)
    extremes = [(2147483647, 9223372036854775807), (-2147483648, -9223372036854775808), (0, 0), (-1, 1), (2147483647, -9223372036854775808), (-2147483648, 999999999999999999),
                (1, 1000000000000000000), (-1, -999999999999999999), (10, -1000000000000000000)]
    for name, fmt in (("compact", b'{"i":%s,"l":%s}'), ("spaced", b'{"i": %s, "l": %s}'), ("unknown", b'{"i":%s,"z":-0,"l":%s}')):
        lines = [fmt % (b"%d" % i, b"%d" % l) for i, l in extremes] + [fmt % (b"-0", b"-0"), fmt % (b"0", b"-0")]
        out.append(("integer_extremes_" + name, lines, [("i", I), ("l", L)]))
    # A-JSON7: bytes that are no UTF-8, copied as they are; the members behind them still parse
    lines = []
    for v in (b"\xff", b"a\xffb", b"\x80", b"lone \x80 here", b"\xe2\x82", b"euro \xe2\x82", b"\xe2\x82\xac", b"\xc3", b"\xf0\x9f\x98", b"\xed\xa0\x80", b"\xc0\xaf"):
        lines += [b'{"b":"%s","a":%d}' % (v, len(lines)), b'{"b": "%s", "a": %d}' % (v, len(lines)), b'{"b":"%s","z":["%s"],"a":%d}' % (v, v, len(lines)),
                  b'{"b":"\\n%s","a":%d}' % (v, len(lines))]
    out.append(("verbatim_bytes", lines, [("b", S), ("a", I)]))
    return [(what, b"\n".join(ls) + b"\n", fields) for what, ls, fields in out]


WELL_FORMED = _well_formed()

# ---- the seeded one-byte mutants --------------------------------------------------------------------------------------------------------------------------------------
MUTANT_FIELDS = [("id", L), ("name", S), ("n", I)]          # (no name is one edit from another: no mutant repeats a key)
MUTANT_GOOD = b'{"id":1,"name":"good","n":2}'
ALPHABET = b'{}[]":,\\ 0123456789e.-tn\t\xc3'


def mutants(seed, count=2000):
    """`count` lines, each ONE byte (deleted, inserted or replaced) away from a well-formed line of one of three writers: compact, Python's separators, and
    compact with a nested member that is not in the schema."""
    rng = np.random.default_rng(7000 + seed)
    words = ["", "plain", "two words, a comma", "q\"uote", "back\\slash", "tab\there", "caf\u00e9", "\u6f22\u5b57", "\U0001F600", "{[:]}", "0123456789", "true", "e-1.5"]
    out = []
    while len(out) < count:
        k = len(out)
        o = {"id": int(rng.integers(-10 ** int(rng.integers(1, 19)), 10 ** int(rng.integers(1, 19)))), "name": words[int(rng.integers(0, len(words)))] + " " + words[k % len(words)],
             "n": int(rng.integers(-2 ** 31, 2 ** 31))}
        writer = k % 3
        if writer == 2:
            items = list(o.items())
            items.insert(int(rng.integers(0, 4)), ("extra", [1, {"k": "}", "t": [True, None, -1.5e3]}, "s"]))
            o = dict(items)
        line = bytearray(json.dumps(o, ensure_ascii=bool(k % 2), separators=(", ", ": ") if writer == 1 else (",", ":")).encode())
        at, op, c = int(rng.integers(0, len(line))), int(rng.integers(0, 3)), ALPHABET[int(rng.integers(0, len(ALPHABET)))]
        if op == 0:
            del line[at]
        elif op == 1:
            line.insert(at, c)
        elif line[at] == c:
            continue
        else:
            line[at] = c
        if b"\n" not in line:                              # (a raw newline would make two lines of it)
            out.append(bytes(line))
    return out


def mutant_text(line):
    """The mutant as line 3 of five."""
    return b"\n".join([MUTANT_GOOD, MUTANT_GOOD, line, MUTANT_GOOD, MUTANT_GOOD]) + b"\n"


# ---- hand-worked lines --------------------------------------------------------------------------------------------------------------------------------------------------
HAND = [
    (b'{"a":1,"b":"x"}', {"a": 1, "b": b"x"}),
    (b' \t{ "b" : "x" ,\t"a" : -7 } \r', {"a": -7, "b": b"x"}),
    (b'{"a":-0,"b":""}', {"a": 0, "b": b""}),
    (b'{"a":2147483647,"b":"\\u00e9\\ud83d\\ude00\\u0000"}', {"a": 2147483647, "b": "\u00e9\U0001F600\0".encode()}),
    (b'{"a":-2147483648,"b":"\\"\\\\\\/\\b\\f\\n\\r\\t"}', {"a": -2147483648, "b": b'"\\/\b\f\n\r\t'}),
    (b'{"a":1,"b":"x","a":2,"b":"y"}', {"a": 2, "b": b"y"}),
    (b'{"z":[1,{"k":"}]"},null],"a":1,"y":-1.5e+3,"b":"x","":{}}', {"a": 1, "b": b"x"}),
    (b'{"a":1,"b":"raw \xc3\xa9 \xff"}', {"a": 1, "b": b"raw \xc3\xa9 \xff"}),
    (b'{"a":1,"b":"x","z":' + b"[" * 64 + b"]" * 64 + b"}", {"a": 1, "b": b"x"}),
    (b'{"a":1,"b":"x","z":' + b"[" * 65 + b"]" * 65 + b"}", "depth"),
    (b"", "blank"), (b" \r", "blank"), (b"{}", "missing"), (b'{"a":1}', "missing"), (b'{"a":1,"b":"x"', "malformed"), (b'{"a":1.0,"b":"x"}', "number"),
    (b'{"a":1.,"b":"x"}', "malformed"), (b'{"a":1x,"b":"x"}', "malformed"), (b'{"a":2147483648,"b":"x"}', "range"), (b'{"a":99999999999.5,"b":"x"}', "number"),
    (b'{"\\u0061":1,"b":"x"}', "key_escape"), (b'{"a":1,"b":"x","z":[1}}', "malformed"), (b'{"a":1,"b":"x","z":NaN}', "malformed"),
    (b'{"a":1,"b":"\\ud800"}', "malformed"), (b'{"a":1,"b":"x"}{"a":1,"b":"x"}', "malformed"),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_worked_lines(case):
    line, want = HAND[case]
    assert check_line(line, AB) == want


def test_the_listed_differences_from_json_loads():
    """The three that check_line lets pass, and the judge's four, each shown once."""
    assert judge(b'{"\\u0061":1,"b":"x"}', AB) == {"a": 1, "b": b"x"} and check_line(b'{"\\u0061":1,"b":"x"}', AB) == "key_escape"
    deep = b'{"a":1,"b":"x","z":' + b"[" * 65 + b"]" * 65 + b"}"
    assert judge(deep, AB) == {"a": 1, "b": b"x"} and check_line(deep, AB) == "depth"
    twice = b'{"a":"no","a":1,"b":"x"}'
    assert judge(twice, AB) == {"a": 1, "b": b"x"}
    with pytest.raises(json_ref._Bad):
        parse_line(twice, AB)
    assert json.loads('{"z":NaN}') and judge(b'{"a":1,"b":"x","z":NaN}', AB) is None
    assert json.loads('"\\ud800"') and judge(b'{"a":1,"b":"\\ud800"}', AB) is None
    assert judge(b'{"a":2147483648,"b":"x"}', AB) is None and judge(b'{"a":2147483648,"b":"x"}', AL) == {"a": 2147483648, "b": b"x"}
    assert judge(b'{"a":1.0,"b":"x"}', AB) is None
    with pytest.raises(UnicodeDecodeError):
        json.loads(b'{"b":"\xff"}')
    assert judge(b'{"a":1,"b":"\xff"}', AB) == {"a": 1, "b": b"\xff"}


def test_lines_and_the_first_offender():
    assert json_ref.lines_of(b"") == [] and json_ref.lines_of(b"x") == [b"x"] and json_ref.lines_of(b"x\n") == [b"x"] and json_ref.lines_of(b"x\n\n") == [b"x", b""]
    assert json_ref.lines_of(b"x\r\ny") == [b"x\r", b"y"] and json_ref.lines_of(b"\n") == [b""]
    cols = decode(b"", AB)
    assert len(cols["a"]) == 0 and cols["a"].dtype == np.int32 and cols["b"].offsets.tolist() == [0]
    cols = decode(GOOD + b"\r\n" + b'{"b":"yz","a":-5}', AL)
    assert cols["a"].tolist() == [1, -5] and cols["a"].dtype == np.int64 and cols["b"].offsets.tolist() == [0, 1, 3] and cols["b"].data.tobytes() == b"xyz"
    with pytest.raises(JsonError) as e:
        decode(GOOD + b"\n" + b'{"a":1.5,"b":"x"}\n' + b'{"a":x}\n', AB)
    assert (e.value.line, e.value.status, e.value.code) == (2, "unsupported", "number") and "line 2: number with a fraction" in str(e.value)
    assert sorted(json_ref.STATUS) == sorted(json_ref.MESSAGES) and len(json_ref.STATUS) == 7


# ---- generated relations ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relation", ["bid", "auction", "person"])
def test_generated_relations(relation):
    cols = _events(relation, 1500)
    text = oracle.nexmark_json_lines(relation, cols)
    fields = SCHEMAS[relation]
    got = decode(text, fields)
    n = 0
    for n, line in enumerate(json_ref.lines_of(text), 1):
        assert isinstance(check_line(line, fields), dict)
    assert n == len(cols[fields[0][0]]) > 0
    for name, t in fields:
        if t == S:
            assert np.array_equal(got[name].offsets, cols[name].offsets) and np.array_equal(got[name].data, cols[name].data[: cols[name].offsets[-1]]), name
        else:
            assert np.array_equal(got[name], cols[name]) and got[name].dtype == cols[name].dtype, name


# ---- the device tests' texts ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(ERRORS)))
def test_errors(case):
    text, fields, (status, line, code) = ERRORS[case]
    assert line != 1
    with pytest.raises(JsonError) as e:
        decode(text, fields)
    assert (e.value.status, e.value.line, e.value.code) == (status, line, code)
    for k, ln in enumerate(json_ref.lines_of(text), 1):
        r = check_line(ln, fields)
        assert r == code if k == line else isinstance(r, dict), (k, ln, r)


@pytest.mark.parametrize("what", [w[0] for w in WELL_FORMED])
def test_well_formed_edges(what):
    _, text, fields = next(w for w in WELL_FORMED if w[0] == what)
    lines = json_ref.lines_of(text)
    assert len(lines) > 8
    for ln in lines:
        assert isinstance(check_line(ln, fields), dict), ln
    decode(text, fields)


@pytest.mark.parametrize("seed", range(4))
def test_mutants(seed):
    """Accept / reject and values against json.loads, and the shares that keep the device differential from going vacuous: the reference refuses at
    least half of a seed's mutants and accepts at least a fifth."""
    lines = mutants(seed)
    assert len(lines) == 2000 and len(set(lines)) > 1900
    assert isinstance(check_line(MUTANT_GOOD, MUTANT_FIELDS), dict)
    codes = {}
    for ln in lines:
        r = check_line(ln, MUTANT_FIELDS)
        codes[r if isinstance(r, str) else "ok"] = codes.get(r if isinstance(r, str) else "ok", 0) + 1
    print(seed, codes)
    rejected = len(lines) - codes.get("ok", 0)
    assert rejected >= 1000 and codes["ok"] >= 400, codes
    assert codes.get("malformed", 0) > 500 and codes.get("missing", 0) > 0 and codes.get("number", 0) > 0, codes     # more than one way to fail
