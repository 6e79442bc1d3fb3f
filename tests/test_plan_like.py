"""Utf8 LIKE / NOT LIKE and ordered Utf8 comparisons in FilterExec (flock_amd/csrc/strmatch.hpp, strmatch.hip; the Words leaf of pred.hpp).

The reference is `reference_like` below -- the pattern cut at `%` into pieces, the first anchored at the start, the last at the end, every middle piece
at its leftmost position; `_` steps over one UTF-8 code point -- checked against a hand-worked table and against pyarrow.compute.match_like (Arrow C++,
the SQL meaning), and Python's `bytes` order for the comparisons.  The GPU tests compare the kept rows, in input order, with the reference applied to the
fed table."""
import json
import os

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")

STAGE_BYTES = 16384      # strmatch.hpp kStrStageBytes: bytes of a value range one round of the `%needle%` kernel holds in LDS
TILE_ROWS = 8192         # scan.hpp kFlagTile
SPLIT_ROWS = 1024        # rows of a group of the staging-round construction: it divides the 2048 rows of a `%needle%` workgroup (scan.hpp kFlagWaveRows)
MAX_PATTERN = 128        # strmatch.hpp kStrMaxPattern
MAX_PERCENT = 16         # strmatch.hpp kStrMaxPieces - 1

COLS = [("s", "Utf8"), ("t", "Utf8"), ("i", "Int32"), ("k", "Int32")]     # k: the row's number (never NULL) -- how the kept rows are told apart
_PA = {"Utf8": pa.string(), "Int32": pa.int32()}


# ------------------------------------------------------------------ the reference
def _pieces(pattern):
    return [p.encode() if isinstance(p, str) else p for p in (pattern.split("%") if isinstance(pattern, str) else pattern.split(b"%"))]


def _is_cont(b):
    return (b & 0xC0) == 0x80


def _fwd(piece, v, p, end):
    """`piece` forwards from byte p of v[:end]: the position after the match, or None"""
    q = p
    for c in piece:
        if q >= end:
            return None
        if c == 0x5F:                       # `_`: one code point
            if _is_cont(v[q]):
                return None
            q += 1
            while q < end and _is_cont(v[q]):
                q += 1
        else:
            if v[q] != c:
                return None
            q += 1
    return q


def _bwd(piece, v, lo, end):
    """`piece` backwards from the end of v[lo:end]: the position of its first byte, or None"""
    q = end
    for c in reversed(piece):
        if q <= lo:
            return None
        q -= 1
        if c == 0x5F:
            while q > lo and _is_cont(v[q]):
                q -= 1
            if _is_cont(v[q]):
                return None
        elif v[q] != c:
            return None
    return q


def reference_like(value: bytes, pattern) -> bool:
    pieces = _pieces(pattern)
    pos = _fwd(pieces[0], value, 0, len(value))
    if pos is None:
        return False
    if len(pieces) == 1:
        return pos == len(value)
    limit = _bwd(pieces[-1], value, pos, len(value))
    if limit is None:
        return False
    for piece in pieces[1:-1]:
        p, found = pos, None
        while p <= limit - len(piece) and found is None:
            found = _fwd(piece, value, p, limit)
            p += 1
        if found is None:
            return False
        pos = found
    return True


_CMP = {"Lt": lambda a, b: a < b, "LtEq": lambda a, b: a <= b, "Gt": lambda a, b: a > b, "GtEq": lambda a, b: a >= b,
        "Eq": lambda a, b: a == b, "NotEq": lambda a, b: a != b}


def test_reference_against_a_hand_worked_table():
    t = [("abc", "abc", True), ("abc", "ab", False), ("abc", "abcd", False), ("abc", "a%", True), ("abc", "%c", True), ("abc", "%b%", True),
         ("abc", "a%c", True), ("abc", "a%b", False), ("ab", "a%b", True), ("a", "a%a", False), ("aa", "a%a", True),
         ("", "", True), ("a", "", False), ("", "%", True), ("abc", "%", True), ("", "%%", True), ("x\ny", "%%", True),
         ("", "_%_", False), ("a", "_%_", False), ("ab", "_%_", True), ("éé", "_%_", True), ("é", "_%_", False),
         ("é", "_", True), ("é", "__", False), ("aé", "a_", True), ("éa", "_a", True), ("€", "_", True), ("a€b", "a_b", True), ("a€b", "a__b", False),
         ("x\ny", "x%y", True), ("x\ny", "x_y", True), ("a\n\nb", "%\n\n%", True),
         ("a.c", "a.c", True), ("abc", "a.c", False), ("a+", "a+", True), ("aa", "a+", False), ("a*", "a*", True), ("aaa", "a*", False),
         ("(a", "(a", True), ("(a", "(%", True), ("a.b.c", "%.%.%", True), ("a.bc", "%.%.%", False),
         ("abcabc", "%abc", True), ("abcab", "%abc", False), ("xaybzc", "%a%b%c", True), ("xaybzc", "%a%c%b", False), ("abab", "ab%ab", True), ("aba", "ab%ba", False),
         ("xabc", "%a_c%", True), ("xaéc", "%a_c%", True), ("xac", "%a_c%", False), ("ba", "_%a%_", False), ("bac", "_%a%_", True), ("ABC", "abc", False)]
    for value, pattern, want in t:
        assert reference_like(value.encode(), pattern) is want, (value, pattern)
    # the trap: a needle that lies across two neighbouring values is in neither
    assert not reference_like(b"..ab", "%bc%") and not reference_like(b"c..", "%bc%")


ALPHABET = ["a", "b", "c", "é", "€", "\n", ".", "+", "*", "("]


def _random_pairs(seed, n, max_value=9, max_pattern=6):
    r = np.random.default_rng(seed)
    pat_alpha = ALPHABET + ["%", "%", "_"]
    out = []
    for _ in range(n):
        v = "".join(r.choice(ALPHABET, r.integers(0, max_value + 1)))
        p = "".join(r.choice(pat_alpha, r.integers(0, max_pattern + 1)))
        out.append((v, p))
    return out


def test_reference_against_arrow_match_like():
    pairs = _random_pairs(11, 24_000)
    by_pattern = {}
    for v, p in pairs:
        by_pattern.setdefault(p, []).append(v)
    compared = matched = 0
    for p, values in by_pattern.items():
        got = pc.match_like(pa.array(values, pa.string()), p).to_pylist()
        for v, g in zip(values, got):
            assert reference_like(v.encode(), p) is g, (v, p, g)
            compared += 1
            matched += g
    assert compared == len(pairs) >= 20_000
    assert 0.02 * compared <= matched <= 0.5 * compared, (matched, compared)


def test_ordered_comparisons_are_bytes_order():
    vals = [b"", b"a", b"ab", b"abc", b"b", b"a\x00", b"a\x00b", "é".encode(), "€".encode(), b"abcdefgh", b"abcdefghi", b"abcdefghijklmnopq", b"\xff"]
    for a in vals:
        for b in vals:
            # a proper prefix sorts first; otherwise the first differing byte decides, as unsigned
            n = min(len(a), len(b))
            k = next((i for i in range(n) if a[i] != b[i]), n)
            lt = (len(a) < len(b)) if k == n else a[k] < b[k]
            assert _CMP["Lt"](a, b) == lt and _CMP["GtEq"](a, b) == (not lt)
            assert _CMP["LtEq"](a, b) == (lt or a == b) and _CMP["Gt"](a, b) == (not lt and a != b)


# ------------------------------------------------------------------ plans
def _field(name, t):
    return {"data_type": t, "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": True}


def col(name, cols=COLS):
    return {"physical_expr": "column", "name": name, "index": [n for n, _ in cols].index(name)}


def lit(v, kind=None):
    if isinstance(v, (str, bytes)):
        return {"physical_expr": "literal", "value": {"Utf8": v.decode() if isinstance(v, bytes) else v}}
    return {"physical_expr": "literal", "value": {kind or "Int32": v}}


def binop(op, l, r):
    return {"physical_expr": "binary_expr", "op": op, "left": l, "right": r}


def like(name, pattern, negated=False, cols=COLS):
    return binop("NotLike" if negated else "Like", col(name, cols), lit(pattern))


def not_(e):
    return {"physical_expr": "not_expr", "arg": e}


def is_null(e):
    return {"physical_expr": "is_null_expr", "arg": e}


def in_list(e, values, negated=False):
    return {"physical_expr": "in_list_expr", "expr": e, "list": [lit(v) for v in values], "negated": negated}


def scan(cols=COLS):
    return {"execution_plan": "memory_exec", "schema": {"fields": [_field(n, t) for n, t in cols], "metadata": {}}, "projection": list(range(len(cols)))}


def filter_plan(pred, cols=COLS, below=None):
    return {"execution_plan": "filter_exec", "predicate": pred, "input": below or scan(cols)}


def evaluate(e, row):
    """SQL three-valued value of predicate / operand `e` over `row` (name -> bytes | int | None): True / False / None, or the operand's value"""
    kind = e["physical_expr"]
    if kind == "column":
        return row[e["name"]]
    if kind == "literal":
        v = list(e["value"].values())[0]
        return v.encode() if isinstance(v, str) else v
    if kind == "cast_expr":
        return evaluate(e["expr"], row)
    if kind == "not_expr":
        v = evaluate(e["arg"], row)
        return None if v is None else not v
    if kind == "is_null_expr":
        return evaluate(e["arg"], row) is None
    if kind == "in_list_expr":
        x = evaluate(e["expr"], row)
        v = None if x is None else any(x == evaluate(i, row) for i in e["list"])
        return None if v is None else (not v if e["negated"] else v)
    op, l, r = e["op"], evaluate(e["left"], row), evaluate(e["right"], row)
    if op in ("And", "Or"):
        if op == "And":
            return False if (l is False or r is False) else (None if (l is None or r is None) else True)
        return True if (l is True or r is True) else (None if (l is None or r is None) else False)
    if l is None or r is None:
        return None
    if op in ("Like", "NotLike"):
        return reference_like(l, r) != (op == "NotLike")
    if op == "Modulo":
        return int(np.fmod(l, r))
    return _CMP[op](l, r)


def expected_rows(pred, table):
    """numbers of the rows of `table` (name -> list of values, None = NULL) the filter keeps, in input order"""
    names = [n for n in table if n != "k"]
    memo, keep = {}, []
    for k, vals in enumerate(zip(*[table[n] for n in names])):
        hit = memo.get(vals)
        if hit is None:
            hit = memo[vals] = evaluate(pred, dict(zip(names, vals))) is True
        if hit:
            keep.append(k)
    return keep


# ------------------------------------------------------------------ CPU: parsing, refusals, stage split
def test_explain_shows_the_predicate():
    from flock_amd.runtime import explain
    assert "Filter(s LIKE 'ab%')" in explain(filter_plan(like("s", "ab%")))
    assert "Filter(s NOT LIKE '%x_y')" in explain(filter_plan(like("s", "%x_y", True)))
    txt = explain(filter_plan(binop("And", binop("Or", like("s", "a%"), is_null(col("s"))), binop("Gt", col("i"), lit(3)))))
    assert "Filter((s LIKE 'a%' OR s IS NULL) AND i > 3)" in txt, txt
    cast = {"physical_expr": "cast_expr", "cast_type": "Utf8", "expr": col("t")}
    assert "t LIKE '%q%'" in explain(filter_plan(binop("Like", cast, lit("%q%"))))
    # ordered comparisons parse, either side; a 64-byte pattern with 8 `%` and the largest one the header allows are taken
    explain(filter_plan(binop("And", binop("GtEq", col("s"), lit("ab")), binop("Lt", lit("zz"), col("s")))))
    explain(filter_plan(like("s", "%".join(["abcdefg"] * 8) + "%")))
    explain(filter_plan(like("s", "%".join(["abcdefgh"] * MAX_PERCENT) + "%")))
    # a filter without LIKE prints as before
    assert "Filter [" in explain(filter_plan(binop("Eq", col("s"), lit("or"))))


@pytest.mark.parametrize("pred,words", [
    (binop("Like", col("i"), lit("1%")), "LIKE on something that is not a Utf8 column"),
    (binop("Like", col("s"), col("t")), "LIKE with a pattern that is not a Utf8 literal"),
    (binop("NotLike", col("s"), lit(7)), "LIKE with a pattern that is not a Utf8 literal"),
    (like("s", "a\\%b"), "LIKE pattern with a backslash"),
    (like("s", "x" * (MAX_PATTERN + 1)), "LIKE pattern beyond"),
    (like("s", "%" * (MAX_PERCENT + 1)), "LIKE pattern beyond"),
    (binop("Eq", like("s", "a%"), like("t", "b%")), "LIKE inside a computed expression"),
    ({"physical_expr": "case_expr", "expr": None, "when_then_expr": [[like("s", "a%"), binop("Gt", col("i"), lit(1))]], "else_expr": None}, "LIKE inside a computed expression"),
])
def test_refusals_name_their_cause(pred, words):
    from flock_amd import FlockGpuError, _ffi
    from flock_amd.runtime import explain
    with pytest.raises(FlockGpuError) as err:
        explain(filter_plan(pred))
    assert err.value.code == _ffi.ERR_UNSUPPORTED and words in str(err.value), str(err.value)


def test_earlier_refusals_keep_their_text():
    from flock_amd import FlockGpuError, _ffi
    from flock_amd.runtime import explain
    with pytest.raises(FlockGpuError) as err:
        explain(json.load(open(os.path.join(PLANS, "unsupported_left_join.json"))))
    assert err.value.code == _ffi.ERR_UNSUPPORTED and "Inner" in str(err.value)
    proj = {"execution_plan": "projection_exec", "input": scan(), "expr": [[like("s", "a%"), "m"]]}
    with pytest.raises(FlockGpuError) as err:
        explain(proj)
    assert "projection of a Boolean expression" in str(err.value)


def _q3_like(pattern="o%"):
    """q3 with the persons' state test made `state LIKE pattern`"""
    plan = json.load(open(os.path.join(PLANS, "q3.json")))

    def walk(n):
        if isinstance(n, dict):
            if n.get("execution_plan") == "filter_exec" and "state" in json.dumps(n["predicate"]):
                c = n["predicate"]
                while c.get("op") == "Or":
                    c = c["left"]
                n["predicate"] = binop("Like", c["left"], lit(pattern))
            for v in n.values():
                walk(v)
        elif isinstance(n, list):
            for v in n:
                walk(v)
    walk(plan)
    return plan


def test_q3_shape_with_like_splits_and_is_not_fused():
    from flock_amd.runtime import explain
    from flock_amd.stages import build_query_dag
    plan = _q3_like()
    txt = explain(plan)
    assert "state LIKE 'o%'" in txt and "fused" not in txt, txt
    assert "fused q3" in explain(json.load(open(os.path.join(PLANS, "q3.json"))))
    stages = build_query_dag(plan)
    assert len(stages) == 3
    texts = [explain(s.plan) for s in stages]
    assert sum("state LIKE 'o%'" in t for t in texts) == 1


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def make_table(s, t=None, i=None):
    """name -> list of values (str -> its UTF-8 bytes; None = NULL)"""
    n = len(s)
    enc = lambda xs: [x.encode() if isinstance(x, str) else x for x in xs]
    return {"s": enc(s), "t": enc(t) if t is not None else [b""] * n, "i": list(i) if i is not None else [0] * n, "k": list(range(n))}


def _array(values, t):
    if t == "Utf8":
        return pa.array(values, pa.binary()).cast(pa.string())
    return pa.array(values, _PA[t])


def batches(table, chunk=1 << 20, cols=COLS):
    n = len(table["k"])
    out = []
    for a in range(0, max(n, 1), chunk):
        out.append(pa.record_batch([_array(table[name][a:a + chunk], t) for name, t in cols], names=[c for c, _ in cols]))
    return out


def run_filter(gpu, pred, table, chunk=1 << 20, generic_only=False, rbs=None):
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([filter_plan(pred)], gpu=gpu, generic_only=generic_only)
    try:
        out = collect(ctx, [[rbs if rbs is not None else batches(table, chunk)]])[0]
    finally:
        ctx.close()
    return [k for b in out for k in b.column(b.schema.get_field_index("k")).to_pylist()], out


def check(gpu, pred, table, chunk=1 << 20, want=None):
    got, out = run_filter(gpu, pred, table, chunk)
    want = expected_rows(pred, table) if want is None else want
    assert len(got) == len(want) and got == want, (json.dumps(pred)[:200], len(got), len(want), [x for x in zip(got, want) if x[0] != x[1]][:5])
    return got, out


def _words(r, n, lo, hi, alphabet="abcdxyz "):
    lens = r.integers(lo, hi + 1, n)
    letters = r.choice(list(alphabet), int(lens.sum()))
    out, p = [], 0
    for L in lens:
        out.append("".join(letters[p:p + L]))
        p += L
    return out


@pytest.mark.gpu
def test_anchored_patterns(gpu):
    r = np.random.default_rng(1)
    s = _words(r, 20_000, 0, 12, "abc") + ["", "a", "ab", "abc", "abcabc", "é", "éa", "aé", "€€", "a€b", "ééé", "ab\ncd", "b", "ba"]
    tab = make_table(s)
    for p in ["ab%", "%ab", "ab", "abc", "a%b", "_b%", "%b_", "_", "__", "_%", "%_", "a_", "_a", "é%", "%é", "_é", "€_", "a_b", "", "%", "%%", "abcabcabcabcabc%",
              "%abcabcabcabcabc", "abcabcabc%abcabcabc", "ab\n%", "___%"]:
        got, _ = check(gpu, like("s", p), tab)
        check(gpu, like("s", p, True), tab)
    assert len(check(gpu, like("s", "%"), tab)[0]) == len(s)
    cast = {"physical_expr": "cast_expr", "cast_type": "Utf8", "expr": col("s")}          # a cast that changes nothing in front of the column
    check(gpu, binop("Like", cast, lit("ab%")), tab)
    # a column of fewer than 8 bytes in all
    tiny = make_table(["a", "", "bc", "a", "é"])
    for p in ["a", "a%", "%c", "_", "b_", "%", "", "_%_"]:
        check(gpu, like("s", p), tiny)


def _contains_table(r, n, lo, hi, needle, rate=0.03):
    s = _words(r, n, lo, hi)
    for k in np.nonzero(r.random(n) < rate)[0]:
        v = s[k]
        at = int(r.integers(0, len(v) + 1))
        s[k] = v[:at] + needle + v[at:]
    return s


NEEDLES = ["q", "qr", "qrs", "qrstuvwx", "qrstuvwxy", "qrstuvwxyzQRSTUVWXYZ0123456789!?#"]


@pytest.mark.gpu
@pytest.mark.parametrize("needle", NEEDLES, ids=[str(len(x)) for x in NEEDLES])
def test_contains_over_short_medium_and_long_values(gpu, needle):
    assert len(needle) in (1, 2, 3, 8, 9, 33)
    r = np.random.default_rng(len(needle))
    pred = like("s", "%" + needle + "%")
    for n, lo, hi in [(30_000, 0, 8), (30_000, 60, 90), (3000, 300, 2000), (40, 20_000, 40_000)]:   # (the last: several staging rounds per value)
        s = _contains_table(r, n, lo, hi, needle)
        s[0] = needle + s[0]                    # at the relation's very first ...
        s[-1] = s[-1] + needle                  # ... and very last bytes
        s[n // 2] = needle                      # a needle equal to a whole value
        # (`in` is what the reference computes for one piece between two `%`: checked on a sample, used for all -- the reference walks bytes in Python)
        want = [k for k, v in enumerate(s) if needle in v]
        tab = make_table(s)
        assert all(reference_like(tab["s"][k], "%" + needle + "%") == (k in set(want[:50])) for k in list(range(0, n, max(n // 200, 1))) if k not in want[50:])
        got, _ = check(gpu, pred, tab, want=want)
        assert 0 in got and n - 1 in got and n // 2 in got and len(got) < n // 2
        hit = set(want)
        check(gpu, like("s", "%" + needle + "%", True), tab, want=[k for k in range(n) if k not in hit])


@pytest.mark.gpu
@pytest.mark.parametrize("needle", ["qr", "qrstuvwxy", NEEDLES[-1]], ids=["2", "9", "33"])
def test_contains_at_every_offset_across_a_staging_round(gpu, needle):
    """Groups of SPLIT_ROWS rows and 3 * STAGE_BYTES bytes, so that every workgroup's byte range (2048 rows: two groups) starts at a multiple of
    STAGE_BYTES; in group g the needle starts `delta` bytes from the group's first round boundary, for every delta from
    "ends two bytes before it" to "starts two bytes after it".  The last value of a group ends with the needle's first h bytes and the next group starts with the
    rest: the trap, which must not match.  Groups cover more than one tile, so the trap also sits on a tile boundary."""
    L = len(needle)
    deltas = list(range(-(L + 2), 3))
    s, want = [], []
    for g, delta in enumerate(deltas * 3):
        h = 1 + g % max(L - 1, 1) if L > 1 else 0
        rows = [needle[h:] + "-" * (48 - (L - h))] + ["-" * 48] * 339          # 340 rows, 16320 bytes: 64 before the boundary
        hit = "." * (64 + delta) + needle + ":::"
        rows.append(hit)
        want.append(len(s) + 340)
        rows += ["=" * 40] * 682
        rest = 3 * STAGE_BYTES - sum(len(x) for x in rows)
        rows.append("~" * (rest - h) + needle[:h])
        assert len(rows) == SPLIT_ROWS and sum(len(x) for x in rows) == 3 * STAGE_BYTES and rest > L
        s += rows
    assert len(s) > 2 * TILE_ROWS
    tab = make_table(s)
    assert expected_rows(like("s", "%" + needle + "%"), tab) == want
    check(gpu, like("s", "%" + needle + "%"), tab, want=want)
    # the classic trap
    check(gpu, like("s", "%bc%"), make_table(["..ab", "c..", "abc", "b", "c", "", "bc"]), want=[2, 6])


@pytest.mark.gpu
def test_general_patterns(gpu):
    r = np.random.default_rng(3)
    s = _words(r, 20_000, 0, 14, "abc") + ["xaybzc", "abc", "aXc", "aéc", "ba", "bac", "a", "", "é", "€a€", "a\nb\nc"]
    s += ["p0q1r2s3t4u5v6w7", "p0 q1 r2 s3 t4 u5 v6 w7 tail", "p0q1r2s3t4u5v6"]
    long64 = "%".join(["abcdefg"] * 8) + "%"
    assert len(long64) == 64
    s += ["abcdefg" * 8, "-".join(["abcdefg"] * 8) + "!", "abcdefg" * 7]
    tab = make_table(s)
    for p in ["%a%b%", "a%b%c", "%a_c%", "_%a%_", "p0%q1%r2%s3%t4%u5%v6%w7", "%p0%q1%r2%s3%t4%u5%v6%w7%", long64, "%a%a%a%a%", "%_b_%", "a%_%c", "%ab%ab%", "%é%", "%_€"]:
        check(gpu, like("s", p), tab)
        check(gpu, like("s", p, True), tab)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(16))
def test_random_patterns_over_random_values(gpu, seed):
    r = np.random.default_rng(100 + seed)
    s = ["".join(r.choice(ALPHABET, r.integers(0, 10))) for _ in range(4096)]
    tab = make_table(s)
    for _, p in _random_pairs(200 + seed, 12):
        check(gpu, like("s", p), tab)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 8191, 8192, 8193, 1_000_037])
def test_sizes(gpu, n):
    r = np.random.default_rng(n % 1000)
    vocab = _words(r, 300, 0, 20) + ["", "qr", "aqrb"]
    s = [vocab[j] for j in r.integers(0, len(vocab), n)]
    tab = make_table(s, i=r.integers(0, 10, n).tolist())
    rbs = batches(tab, 400_000)
    for pred in [like("s", "%qr%"), like("s", "a%"), like("s", "%a%b%"), binop("Gt", col("s"), lit("c")), binop("And", like("s", "%b%", True), binop("Lt", col("i"), lit(5)))]:
        got, _ = run_filter(gpu, pred, tab, rbs=rbs)
        assert got == expected_rows(pred, tab)


@pytest.mark.gpu
def test_a_relation_the_streaming_instances_take(gpu):
    """More than 4 tiles per compute unit (256 CUs): no (tiles, 8) split, the ragged last tile in a launch of its own."""
    n = 4 * 256 * TILE_ROWS + 4097
    r = np.random.default_rng(8)
    vocab = _words(r, 500, 0, 9) + ["", "qr", "aqrb", "bqr"]
    idx = r.integers(0, len(vocab), n)
    arr = pa.array(vocab, pa.string()).take(pa.array(idx))
    rb = pa.record_batch([arr, pa.array([""], pa.string()).take(pa.array(np.zeros(n, np.int64))), pa.array((idx % 7).astype(np.int32)), pa.array(np.arange(n, dtype=np.int32))],
                         names=[c for c, _ in COLS])
    enc = [v.encode() for v in vocab]
    for pred in [like("s", "%qr%"), like("s", "_b%"), like("s", "%a%b%"), binop("LtEq", col("s"), lit("b")), binop("And", like("s", "%c%"), binop("Eq", binop("Modulo", col("i"), lit(3)), lit(1)))]:
        per_value = {(v, m): evaluate(pred, {"s": v, "t": b"", "i": m}) is True for v in set(enc) for m in range(7)}
        keep = np.array([[per_value[(v, m)] for m in range(7)] for v in enc])
        want = np.nonzero(keep[idx, idx % 7])[0]
        got, _ = run_filter(gpu, pred, None, rbs=[rb.slice(a, 3_000_000) for a in range(0, n, 3_000_000)])
        assert np.array_equal(np.asarray(got), want), json.dumps(pred)[:120]


def _null_table(n, seed, null_s=0.2, null_i=0.2):
    r = np.random.default_rng(seed)
    s = _words(r, n, 0, 6, "abc")
    t = _words(r, n, 0, 6, "abc")
    i = r.integers(0, 8, n).tolist()
    s = [None if x else v for v, x in zip(s, r.random(n) < null_s)]
    i = [None if x else v for v, x in zip(i, r.random(n) < null_i)]
    return make_table(s, t, i)


@pytest.mark.gpu
def test_nulls(gpu):
    tab = _null_table(30_000, 5)
    for pred in [like("s", "a%"), like("s", "a%", True), not_(like("s", "a%")), like("s", "%b%"), like("s", "%b%", True), like("s", "%a%b%", True),
                 binop("Or", like("s", "a%"), is_null(col("s"))), binop("Or", like("s", "%b%", True), is_null(col("s"))),
                 binop("And", like("s", "%b%"), binop("Gt", col("i"), lit(3))), binop("Or", like("s", "%b%"), binop("Gt", col("i"), lit(3))),
                 not_(binop("And", like("s", "a%"), binop("Gt", col("i"), lit(3)))), like("s", "%"), like("s", "%", True),
                 binop("Lt", col("s"), lit("b")), not_(binop("GtEq", col("s"), lit("b")))]:
        got, _ = check(gpu, pred, tab, chunk=7001)
    n_null = sum(v is None for v in tab["s"])
    assert n_null > 1000 and len(check(gpu, like("s", "%"), tab)[0]) == len(tab["k"]) - n_null
    assert len(check(gpu, binop("Or", like("s", "a%"), is_null(col("s"))), tab)[0]) > n_null


@pytest.mark.gpu
def test_validity_through_a_feed_of_several_batches(gpu):
    """NULLs in the second and fourth batch only: the column's validity bytes start with the first batch that holds one"""
    tab = _null_table(20_000, 6, null_s=0.0, null_i=0.0)
    for k in list(range(5000, 10_000, 3)) + list(range(15_000, 20_000, 7)):
        tab["s"][k] = None
    for pred in [like("s", "%b%"), like("s", "a%", True), binop("Or", like("s", "%b%"), is_null(col("s"))), binop("GtEq", col("s"), lit("b"))]:
        check(gpu, pred, tab, chunk=5000)


@pytest.mark.gpu
def test_composition_with_the_other_leaves(gpu):
    tab = _null_table(40_000, 7, null_s=0.1, null_i=0.1)
    mod = binop("Eq", binop("Modulo", col("i"), lit(3)), lit(1))
    preds = [binop("And", like("s", "%b%"), binop("Eq", col("t"), lit("ab"))),
             binop("Or", like("s", "a%"), in_list(col("t"), ["a", "b", "abc"])),
             binop("And", binop("And", like("s", "%a%"), mod), binop("LtEq", col("i"), lit(5))),
             binop("And", like("s", "a%"), like("s", "%c")), binop("Or", like("s", "%ab%"), like("s", "%ba%", True)),
             binop("And", like("s", "%a%"), like("t", "%b%")), binop("Or", like("s", "b_%"), like("t", "%c%c%")),
             binop("And", binop("GtEq", col("s"), lit("ab")), binop("Lt", col("s"), lit("b"))),
             binop("And", binop("Or", like("s", "%c%"), in_list(col("s"), ["a", ""], True)), not_(binop("And", mod, like("t", "_%"))))]
    for pred in preds:
        want = check(gpu, pred, tab)[0]
        assert run_filter(gpu, pred, tab, generic_only=True)[0] == want


def _q3_relations(n_person, n_auction, seed):
    r = np.random.default_rng(seed)
    states = ["or", "id", "ca", "oh", "ok", "wa", "o", ""]
    person = pa.record_batch([pa.array(np.arange(n_person, dtype=np.int32) + 1000), pa.array(_words(r, n_person, 3, 12)), pa.array(_words(r, n_person, 3, 9)),
                              pa.array([states[j] for j in r.integers(0, len(states), n_person)])], names=["p_id", "name", "city", "state"])
    auction = pa.record_batch([pa.array(np.arange(n_auction, dtype=np.int32) + 5000), pa.array((r.integers(0, n_person, n_auction) + 1000).astype(np.int32)),
                               pa.array(r.integers(8, 13, n_auction).astype(np.int32))], names=["a_id", "seller", "category"])
    return {"auction": auction, "person": person}


def _rows(bs):
    out = []
    for rb in bs:
        out.extend(zip(*[rb[c].to_pylist() for c in rb.schema.names]))
    return sorted(out)


@pytest.mark.gpu
def test_filter_under_a_join_whole_and_staged(gpu):
    from flock_amd import stages as S
    from flock_amd.runtime import ExecutionContext, collect
    rel = _q3_relations(30_000, 90_000, 9)
    p, a = rel["person"], rel["auction"]
    keep = {pid: (nm, c, st) for pid, nm, c, st in zip(p["p_id"].to_pylist(), p["name"].to_pylist(), p["city"].to_pylist(), p["state"].to_pylist())
            if reference_like(st.encode(), "o%")}
    want = sorted(keep[sl] + (aid,) for aid, sl, cat in zip(a["a_id"].to_pylist(), a["seller"].to_pylist(), a["category"].to_pylist()) if cat == 10 and sl in keep)
    assert len(want) > 1000
    plan = _q3_like()
    for generic_only in (False, True):
        ctx = ExecutionContext([plan], gpu=gpu, generic_only=generic_only)
        try:
            assert _rows(collect(ctx, [[[a]], [[p]]])[0]) == want
        finally:
            ctx.close()
    for dev in (False, True):     # the boundary through the host, and in HBM
        run = S.StagedRun(gpu, S.build_query_dag(plan), instances=1, on_device=dev)
        try:
            assert _rows(run.run({"auction": a, "person": p})) == want, dev
        finally:
            run.close()


@pytest.mark.gpu
def test_ordered_comparisons(gpu):
    r = np.random.default_rng(10)
    s = _words(r, 20_000, 0, 20, "ab") + ["", "a", "ab", "abababab", "ababababa", "abababababababab", "ababababababababa", "b", "a\x00", "a\x00b", "\x00", "é", "€", "ab\x00"]
    s = [None if x else v for v, x in zip(s, r.random(len(s)) < 0.1)]
    tab = make_table(s)
    for literal in ["", "a", "ab", "abababab", "ababababa", "abababababababab", "ababababababababa", "abababababababababababab", "b", "a\x00", "é", "zz"]:
        for op in ["Lt", "LtEq", "Gt", "GtEq"]:
            check(gpu, binop(op, col("s"), lit(literal)), tab)
        check(gpu, binop("Lt", lit(literal), col("s")), tab)       # a literal on the left swaps the operator
        check(gpu, binop("GtEq", lit(literal), col("s")), tab)
