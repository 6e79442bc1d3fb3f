"""Text slice functions (flock_amd/csrc/textslice.hpp A-SL1..A-SL8): split_part, left, right, ltrim, rtrim, btrim of a Utf8 column as projected columns,
CASE branches, GROUP BY / ORDER BY / DISTINCT keys and COUNT(DISTINCT) arguments, nested, over filters and joins and in stage plans.  Every GPU comparison
is value for value against tests/text_slice_ref.py (NULLs as NULLs, '' as ''), the input fed in uneven batches."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import scalar_fn_ref as sref
import text_slice_ref as ref
from scalar_fn_ref import fn
from text_expr_ref import case, lit_null, lit_utf8
from text_slice_ref import lit, sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")

ROWS = 1024          # textslice.hpp kSliceRows: rows of a workgroup of the streaming kernel
ROUND = 32768        # textslice.hpp kSliceRoundBytes: bytes of one round
TILE = 1024          # textsel.hpp kTextTile: rows of a workgroup of the length and emit kernels

COLS = [("k", "Int32"), ("i", "Int32"), ("s", "Utf8"), ("u", "Utf8")]
TYPES = dict(COLS)
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "Utf8": pa.string()}


def _field(name, t, nullable=True):
    return {"data_type": t, "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


def c(name, cols=COLS):
    return {"physical_expr": "column", "name": name, "index": [n for n, _ in cols].index(name)}


def binary(l, op, r):
    return {"physical_expr": "binary_expr", "left": l, "op": op, "right": r}


def cast(e, t):
    return {"physical_expr": "cast_expr", "expr": e, "cast_type": t}


def mod(col, m, r):
    return binary(binary(c(col), "Modulo", lit("Int32", m)), "Eq", lit("Int32", r))


def split(e, d, n):
    return sl("split_part", e, lit("Utf8", d), lit("Int64", n))


def left(e, n):
    return sl("left", e, lit("Int64", n))


def right(e, n):
    return sl("right", e, lit("Int64", n))


def trim(which, e, chars=None):
    return sl(which, e) if chars is None else sl(which, e, lit("Utf8", chars))


def scan(cols=COLS):
    return {"execution_plan": "memory_exec", "schema": {"fields": [_field(n, t) for n, t in cols], "metadata": {}}, "projection": list(range(len(cols)))}


def projection(exprs, inp=None, types=None):
    """exprs: (expression, name); a computed column is Utf8."""
    types = TYPES if types is None else types
    ty = lambda e: types[e["name"]] if e.get("physical_expr") == "column" else "Utf8"
    return {"execution_plan": "projection_exec", "expr": [[e, n] for e, n in exprs], "input": scan() if inp is None else inp,
            "schema": {"fields": [_field(n, ty(e)) for e, n in exprs], "metadata": {}}}


def filter_(pred, inp=None):
    return {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096, "input": {"execution_plan": "filter_exec", "predicate": pred, "input": scan() if inp is None else inp}}


def sort_(inp, keys):
    return {"execution_plan": "sort_exec", "input": inp, "expr": [{"expr": e, "options": {"descending": d, "nulls_first": False}} for e, d in keys]}


def group_by(key_expr, parts=None, key="label", count_arg=None):
    """SELECT <key>, COUNT(*), COUNT(<count_arg or key>) GROUP BY 1 -- Partial / [Hash] / Final."""
    aggs = [{"aggregate_expr": "count", "name": "COUNT(UInt8(1))", "data_type": "UInt64", "nullable": True, "expr": lit("UInt8", 1)},
            {"aggregate_expr": "count", "name": "COUNT(x)", "data_type": "UInt64", "nullable": True, "expr": key_expr if count_arg is None else count_arg}]
    ins = {"fields": [_field(n, t) for n, t in COLS], "metadata": {}}
    kc = {"physical_expr": "column", "name": key, "index": 0}
    partial = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [[key_expr, key]], "aggr_expr": aggs, "input": scan(), "input_schema": ins,
               "schema": {"fields": [_field(key, "Utf8"), _field("COUNT(UInt8(1))[count]", "UInt64"), _field("COUNT(x)[count]", "UInt64")], "metadata": {}}}
    mid = partial
    if parts:
        mid = {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096,
               "input": {"execution_plan": "repartition_exec", "input": partial, "partitioning": {"Hash": [[kc], parts]}}}
    return {"execution_plan": "hash_aggregate_exec", "mode": "FinalPartitioned" if parts else "Final", "group_expr": [[kc, key]], "aggr_expr": aggs, "input": mid, "input_schema": ins,
            "schema": {"fields": [_field(key, "Utf8"), _field("COUNT(UInt8(1))", "UInt64"), _field("COUNT(x)", "UInt64")], "metadata": {}}}


def distinct(key_expr, key="x"):
    """SELECT DISTINCT <key>: a GROUP BY with no aggregate."""
    ins = {"fields": [_field(n, t) for n, t in COLS], "metadata": {}}
    out = {"fields": [_field(key, "Utf8")], "metadata": {}}
    kc = {"physical_expr": "column", "name": key, "index": 0}
    part = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [[key_expr, key]], "aggr_expr": [], "input": scan(), "input_schema": ins, "schema": out}
    rep = {"execution_plan": "repartition_exec", "input": part, "partitioning": {"Hash": [[kc], 4]}}
    return {"execution_plan": "hash_aggregate_exec", "mode": "FinalPartitioned", "group_expr": [[kc, key]], "aggr_expr": [], "input": rep, "input_schema": ins, "schema": out}


def count_distinct(arg):
    """SELECT COUNT(DISTINCT <arg>), COUNT(*) -- ungrouped, Partial / Final read as one pass."""
    entries = [{"aggregate_expr": "distinct_count", "name": "COUNT(DISTINCT x)", "data_type": "UInt64", "nullable": True, "exprs": [arg], "state_data_types": ["Utf8"], "input_data_types": ["Utf8"]},
               {"aggregate_expr": "count", "name": "COUNT(x)", "data_type": "UInt64", "nullable": True, "expr": lit("UInt8", 1)}]
    ins = {"fields": [_field(n, t) for n, t in COLS], "metadata": {}}
    partial = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [], "aggr_expr": entries, "input": scan(), "input_schema": ins, "schema": {"fields": [], "metadata": {}}}
    return {"execution_plan": "hash_aggregate_exec", "mode": "Final", "group_expr": [], "aggr_expr": entries, "input": {"execution_plan": "coalesce_partitions_exec", "input": partial},
            "input_schema": ins, "schema": {"fields": [_field("COUNT(DISTINCT x)", "UInt64"), _field("COUNT(x)", "UInt64")], "metadata": {}}}


# values with 1- to 4-byte code points, delimiters at their ends, adjacent delimiters, blanks and tabs around them
WORDS = ["", " ", "a", "/", "//", "a/b", "/a/b/", "a//b/c", "été/€/\U0001F600", "  padded  ", "\t tab \t", "xxleftxx", "x" * 15 + "/", "y" * 16 + "/z", "/" + "w" * 17,
         "http://host/d1/d2/file.html", "a,b , c", "~@~a~@~~@~b", "aaaa", "é€\U0001F600é€", " é ", "€€x€€", "q" * 70 + " " + "r" * 3]


def make_table(n, seed, null_p=0.15):
    r = np.random.default_rng(seed)
    nul = lambda xs: [None if r.random() < null_p else x for x in xs]
    return {"k": list(range(n)), "i": nul([int(x) for x in r.integers(-40, 400, n)]),
            "s": nul([WORDS[int(x)] + ("%d" % x if x % 3 == 0 else "") for x in r.integers(0, len(WORDS), n)]),
            "u": nul([" " * int(x % 3) + "u%d/v%d" % (x, x % 7) + " " * int(x % 2) for x in r.integers(0, 50, n)])}


_TABLES = {}


def shared_table(n, null_p=0.15):
    if (n, null_p) not in _TABLES:
        _TABLES[(n, null_p)] = make_table(n, 500 + n, null_p)
    return _TABLES[(n, null_p)]


def batches(t, chunk, cols=COLS):
    n = len(t[cols[0][0]])
    return [pa.record_batch([pa.array(t[cn][a:a + chunk], _PA[ty]) for cn, ty in cols], names=[cn for cn, _ in cols]) for a in range(0, max(n, 1), max(chunk, 1))]


def uneven(t, sizes, cols=COLS):
    """The table in batches of the given sizes over and over."""
    n = len(t[cols[0][0]])
    out, a, j = [], 0, 0
    while a < n or not out:
        b = min(n, a + sizes[j % len(sizes)])
        out.append(pa.record_batch([pa.array(t[cn][a:b], _PA[ty]) for cn, ty in cols], names=[cn for cn, _ in cols]))
        a, j = max(b, a + 1), j + 1
    return out


def refused(plan, *words):
    from flock_amd import _ffi
    from flock_amd.runtime import FlockGpuError, explain
    with pytest.raises(FlockGpuError) as e:
        explain(plan)
    assert e.value.code == _ffi.ERR_UNSUPPORTED, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


# every kind of call once: the streaming kernel's three classes with constant and per-row k, the general kernel's two
EVERY = [split(c("s"), "/", 1), split(c("s"), "/", 2), split(c("s"), "/", 4), left(c("s"), 3), left(c("s"), -2), right(c("s"), 2), right(c("s"), -1), right(c("s"), 0),
         trim("ltrim", c("s")), trim("rtrim", c("s")), trim("btrim", c("u")), trim("btrim", c("s"), " x/\t"), split(c("s"), "~@~", 2), trim("btrim", c("s"), " é€")]


# ------------------------------------------------------------------ CPU: the reference
def test_reference_by_hand():
    assert ref.split_part("abc~@~def~@~ghi", "~@~", 2) == "def"
    assert ref.split_part("aaa", "aa", 2) == "a" and ref.split_part("aaa", "aa", 1) == "" and ref.split_part("aaaa", "aa", 3) == ""
    assert ref.split_part("a/b", "/", 3) == "" and ref.split_part("a/b", "/", 2) == "b" and ref.split_part("", "/", 1) == "" and ref.split_part("//", "/", 2) == ""
    assert ref.left("été€", -1) == "été" and ref.right("été€", 2) == "é€" and ref.left("été€", 2) == "ét" and ref.right("été€", -1) == "té€"
    assert ref.left("abc", 0) == "" and ref.left("abc", 5) == "abc" and ref.left("abc", -3) == "" and ref.left("abc", -7) == ""
    assert ref.right("abc", 0) == "" and ref.right("", 0) == "" and ref.right("abc", 5) == "abc" and ref.right("abc", -3) == "" and ref.right("abc", -7) == ""
    assert ref.ltrim("\t a ") == "\t a " and ref.ltrim(" \ta ") == "\ta " and ref.rtrim(" a \t") == " a \t" and ref.btrim("  a  ") == "a"
    assert ref.ltrim("xyxa", "yx") == "a" and ref.rtrim("€aé€", "€é") == "€a" and ref.btrim("abc", "") == "abc" and ref.btrim("   ") == ""
    t = {"s": ["a/b/c", None, "", " x "]}
    assert ref.eval_text(split(c("s"), "/", 2), t, TYPES) == ["b", None, "", ""]
    assert ref.eval_text(trim("btrim", split(c("s"), "/", 1)), t, TYPES) == ["a", None, "", "x"]
    assert ref.eval_text(cast(left(cast(c("s"), "Utf8"), 2), "Utf8"), t, TYPES) == ["a/", None, "", " x"]


def _random_values(seed, n=3000):
    r = np.random.default_rng(seed)
    alphabet = ["a", "b", " ", "/", "x", "é", "ß", "€", "中", "\U0001F600", "\U00010348", "\t"]
    out = []
    for _ in range(n):
        if r.random() < 0.1:
            out.append(None)
        else:
            out.append("".join(alphabet[int(j)] for j in r.integers(0, len(alphabet), int(r.integers(0, 12)))))
    out[:3] = ["", None, " "]
    return out


@pytest.mark.parametrize("seed", range(3))
def test_reference_against_pyarrow(seed):
    vals = _random_values(40 + seed)
    arr = pa.array(vals, pa.string())
    ap = lambda f, *a: [None if v is None else f(v, *a) for v in vals]
    assert any(v is None for v in vals) and "" in vals and any(len(v.encode()) > len(v) + 4 for v in vals if v)
    for n in (0, 1, 2, 5, 11, 12, 40):
        assert pc.utf8_slice_codeunits(arr, 0, n).to_pylist() == ap(ref.left, n)
        if n:
            assert pc.utf8_slice_codeunits(arr, 0, -n).to_pylist() == ap(ref.left, -n)
            assert pc.utf8_slice_codeunits(arr, -n).to_pylist() == ap(ref.right, n)
            assert pc.utf8_slice_codeunits(arr, n).to_pylist() == ap(ref.right, -n)
    assert ap(ref.right, 0) == [None if v is None else "" for v in vals]
    for chars in (" ", "a ", "é€", " \U0001F600b/", "x"):
        assert pc.utf8_ltrim(arr, characters=chars).to_pylist() == ap(ref.ltrim, chars)
        assert pc.utf8_rtrim(arr, characters=chars).to_pylist() == ap(ref.rtrim, chars)
        assert pc.utf8_trim(arr, characters=chars).to_pylist() == ap(ref.btrim, chars)
    for d in ("/", " ", "é", "a ", "  ", "€中"):
        lists = pc.split_pattern(arr, pattern=d).to_pylist()
        for n in (1, 2, 3, 7):
            assert [None if l is None else (l[n - 1] if n <= len(l) else "") for l in lists] == ap(ref.split_part, d, n)


# ------------------------------------------------------------------ CPU: parsing, explain, refusals
def test_every_function_explains_with_its_arguments():
    from flock_amd.runtime import explain
    for e, text in ((split(c("s"), "/", 4), "split_part(s, '/', 4)"), (left(c("s"), 3), "left(s, 3)"), (left(c("s"), -2), "left(s, -2)"), (right(c("u"), 8), "right(u, 8)"),
                    (trim("ltrim", c("s")), "ltrim(s)"), (trim("rtrim", c("s"), "xy "), "rtrim(s, 'xy ')"), (trim("btrim", c("s"), "é€"), "btrim(s, 'é€')"),
                    (trim("btrim", c("s"), ""), "btrim(s, '')"), (split(c("s"), "~@~", 2), "split_part(s, '~@~', 2)"),
                    (sl("SPLIT_PART", cast(c("s"), "Utf8"), cast(lit("Utf8", "/"), "Utf8"), cast(lit("Int64", 2), "Int64")), "split_part(s, '/', 2)"),
                    (sl("Left", c("s"), lit("Int32", 2), return_type=None), "left(s, 2)")):
        first = explain(projection([(e, "x"), (c("k"), "k")])).splitlines()[0]
        assert first.startswith("Project(x = %s) [x:Utf8, k:Int32]" % text), first
    assert explain(projection([(split(c("s"), "/", 4), "dir1")])).splitlines()[0].startswith("Project(dir1 = split_part(s, '/', 4)) [dir1:Utf8]")


def test_nested_calls_case_and_keys_explain():
    from flock_amd.runtime import explain
    nested = trim("btrim", split(c("s"), ",", 1))
    assert explain(projection([(nested, "x")])).splitlines()[0].startswith("Project(x = btrim(split_part(s, ',', 1))) [x:Utf8]")
    four = trim("rtrim", trim("ltrim", left(split(c("s"), "/", 2), 5)), "x")
    assert "x = rtrim(ltrim(left(split_part(s, '/', 2), 5)), 'x')" in explain(projection([(four, "x")]))
    in_case = case([(mod("i", 2, 0), split(c("s"), "/", 1)), (mod("i", 3, 0), lit_utf8("three"))], trim("btrim", c("u")))
    assert explain(projection([(in_case, "x")])).splitlines()[0].startswith("Project(x = CASE ...) [x:Utf8]")
    # sixteen sources: identical slices count once, different ones each
    many = lambda k: case([(mod("i", 100, j), split(c("s"), "/", j + 1)) for j in range(k - 1)] + [(mod("i", 100, 50), split(c("s"), "/", 1))], c("s"))
    assert "x:Utf8" in explain(projection([(many(16), "x")]))
    refused(projection([(many(17), "x")]), "more than 16 distinct sources")
    txt = explain(group_by(split(c("u"), "/", 2), parts=4))
    assert "Aggregate(Partial)" in txt and "#4:Utf8" in txt and "Project(#4 = split_part(u, '/', 2), #5 = split_part(u, '/', 2))" in txt, txt
    txt = explain(sort_(scan(), [(right(c("s"), 2), True), (c("k"), False)]))
    assert "Sort(#4 DESC, k ASC)" in txt and "Project(#4 = right(s, 2))" in txt, txt
    assert "#4:Utf8" in explain(count_distinct(trim("btrim", c("u"))))
    assert "Project(#4 = left(s, 1))" in explain(distinct(left(c("s"), 1)))


def test_both_fixtures_explain_and_are_not_fused_queries():
    from flock_amd import _ffi, build
    from flock_amd.runtime import explain
    raw = open(os.path.join(PLANS, "q22_url_dirs.json")).read()
    txt = explain(raw)
    assert txt.splitlines()[0].startswith("Project(dir1 = split_part(url, '/', 4), dir2 = split_part(url, '/', 5)) [auction:Int32, bidder:Int32, price:Int32, dir1:Utf8, dir2:Utf8]"), txt
    raw2 = open(os.path.join(PLANS, "person_email_domains.json")).read()
    txt2 = explain(raw2)
    assert "= split_part(email_address, '@', 2))" in txt2 and txt2.splitlines()[0].startswith("Project [domain:Utf8, COUNT(UInt8(1)):UInt64]"), txt2
    assert "fused" not in txt and "fused" not in txt2
    build.build()
    lib = _ffi.load()
    for text in (raw, raw2):
        got = C.c_int(-1)
        assert lib.flockgpu_plan_recognise(text.encode(), len(text.encode()), C.byref(got)) == _ffi.OK and got.value == 0


def test_refusals_by_name():
    p = lambda e: projection([(e, "x")])
    start = lambda name: "scalar_function_expr: function '%s'" % name
    # a column or computed n / delim / chars
    refused(p(sl("split_part", c("s"), c("u"), lit("Int64", 1))), start("split_part"), "the delimiter is a column")
    refused(p(sl("split_part", c("s"), lit("Utf8", "/"), c("i"))), start("split_part"), "n is a column")
    refused(p(sl("left", c("s"), binary(c("i"), "Plus", lit("Int32", 1)))), start("left"), "n is a computed value")
    refused(p(sl("right", c("s"), c("i"))), start("right"), "n is a column")
    refused(p(sl("ltrim", c("s"), c("u"))), start("ltrim"), "the characters is a column")
    refused(p(sl("left", c("s"), lit("Utf8", "3"))), start("left"), "n is not an integer literal")
    refused(p(sl("rtrim", c("s"), lit("Int64", 3))), start("rtrim"), "the characters is not a Utf8 literal")
    # a NULL literal argument
    refused(p(sl("split_part", c("s"), lit_null("Utf8"), lit("Int64", 1))), start("split_part"), "a NULL literal as the delimiter")
    refused(p(sl("left", c("s"), lit_null("Int64"))), start("left"), "a NULL literal as n")
    refused(p(sl("btrim", c("s"), lit_null())), start("btrim"), "a NULL literal as the characters")
    # the value argument
    refused(p(sl("left", lit_utf8("abc"), lit("Int64", 1))), start("left"), "the value argument is a literal")
    refused(p(sl("btrim", case([(mod("i", 2, 0), c("s"))], c("u")))), start("btrim"), "the value argument is a CASE")
    refused(p(sl("rtrim", c("i"))), start("rtrim"), "the value argument is a column that is not Utf8")
    refused(p(sl("ltrim", lit_null("Utf8"))), start("ltrim"), "the value argument is a literal")
    # argument counts
    refused(p(sl("split_part", c("s"), lit("Utf8", "/"))), start("split_part"), "with 2 arguments")
    refused(p(sl("left", c("s"))), start("left"), "with 1 arguments")
    refused(p(sl("right", c("s"), lit("Int64", 1), lit("Int64", 1))), start("right"), "with 3 arguments")
    refused(p(sl("btrim")), start("btrim"), "with 0 arguments")
    refused(p(sl("ltrim", c("s"), lit("Utf8", " "), lit("Utf8", " "))), start("ltrim"), "with 3 arguments")
    # the limits
    refused(p(split(c("s"), "/", 0)), start("split_part"), "n = 0")
    refused(p(split(c("s"), "/", -1)), start("split_part"), "n = -1")
    refused(p(split(c("s"), "", 1)), start("split_part"), "an empty delimiter")
    refused(p(split(c("s"), "d" * 17, 1)), start("split_part"), "a delimiter of more than 16 bytes")
    refused(p(split(c("s"), "€" * 6, 1)), start("split_part"), "a delimiter of more than 16 bytes")
    refused(p(trim("btrim", c("s"), "abcdefghijklmnopq")), start("btrim"), "more than 16 characters")
    refused(p(left(c("s"), 2**31)), start("left"), "n beyond Int32")
    refused(p(right(c("s"), -2**31 - 1)), start("right"), "n beyond Int32")
    five = trim("btrim", trim("ltrim", trim("rtrim", left(right(c("s"), 9), 8))))
    refused(p(five), start("btrim"), "nested more than 4 deep")
    refused(p(sl("left", c("s"), lit("Int64", 1), return_type="Int32")), start("left"), "return_type is not the function's Utf8")
    refused(p(sl("btrim", c("s"), return_type="LargeUtf8")), start("btrim"), "return_type")
    # ... and what is inside the limits is taken
    from flock_amd.runtime import explain
    for e in (split(c("s"), "d" * 16, 2**31 - 1), trim("ltrim", c("s"), "abcdefghijklmnop"), trim("rtrim", c("s"), "é" * 16), left(c("s"), -2**31), right(c("s"), 2**31 - 1),
              trim("btrim", trim("ltrim", trim("rtrim", left(c("s"), 8))))):
        assert "x:Utf8" in explain(p(e))


def test_what_stays_refused_keeps_its_message():
    p = lambda e: projection([(e, "x")])
    for name in ("substr", "lower", "upper", "trim", "concat"):
        refused(p(sl(name, c("s"))), "scalar_function_expr: function '%s' produces text: not yet" % name)
    refused(p(sl("soundex", c("s"))), "scalar_function_expr: function 'soundex' is not supported")
    # octet_length / char_length take a column only; LIKE takes a column only; a slice is no numeric value
    refused(projection([(fn("char_length", left(c("s"), 2)), "x")]), "function 'char_length'", "not a Utf8 column")
    refused(projection([(fn("octet_length", trim("btrim", c("s"))), "x")]), "function 'octet_length'", "not a Utf8 column")
    refused(filter_(binary(left(c("s"), 2), "Like", lit_utf8("a%"))), "LIKE on something that is not a Utf8 column")
    refused(projection([(case([(mod("i", 2, 0), left(c("s"), 2))], lit("Int32", 3)), "x")]), "CASE branches of different types")
    for f in ("min", "max"):
        agg = {"aggregate_expr": f, "name": "M", "data_type": "Utf8", "nullable": True, "expr": left(c("s"), 2)}
        plan = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [], "aggr_expr": [agg], "input": scan(),
                "input_schema": {"fields": [_field(n, t) for n, t in COLS], "metadata": {}}, "schema": {"fields": [_field("M[%s]" % f, "Utf8")], "metadata": {}}}
        refused(plan, f + " needs an integer column")


def test_the_bit_helpers_on_the_host():
    """textslice_bits.hpp (the masks of a chunk, the k-th / last set bit) as a stand-alone host program, under the address and undefined-behaviour sanitizers."""
    exe = os.path.join(ROOT, "tests", "cpp", "textslice_bits_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "flock_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "textslice_bits_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "textslice_bits_test: ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    ctx = GpuContext(0)
    yield ctx
    ctx.close()


def run(gpu, plan, sources, chunk=7_000):
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        return collect(ctx, [[bs if isinstance(bs, list) else batches(bs, chunk, cl)] for bs, cl in sources])[0][0]
    finally:
        ctx.close()


def raw_bytes(col):
    """(validity as values, offsets, data) of a Utf8 result column: what 'identical bytes' compares."""
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    offs = np.frombuffer(col.buffers()[1], dtype=np.int32)[col.offset:col.offset + len(col) + 1]
    data = col.buffers()[2].to_pybytes()[int(offs[0]):int(offs[-1])] if len(col) and col.buffers()[2] is not None else b""
    return col.is_valid().to_pylist(), (offs - offs[0]).tolist() if len(offs) else [], data


def check(gpu, exprs, t, chunk=7_000, srcs=None, cols=COLS, types=TYPES):
    """Projects k and every expression; each column equals the reference value for value, NULLs as NULLs, '' as ''."""
    plan = projection([(c("k", cols), "k")] + [(e, "x%d" % j) for j, e in enumerate(exprs)], inp=scan(cols), types=types)
    rb = run(gpu, plan, [(srcs if srcs is not None else t, cols)], chunk)
    n = len(t["k"])
    assert rb.num_rows == n and rb.column(0).to_pylist() == t["k"]
    for j, e in enumerate(exprs):
        want = pa.array(ref.eval_text(e, t, types), pa.string())
        got = rb.column(1 + j)
        assert got.type == pa.string()
        assert got.equals(want), (j, json.dumps(e)[:200], [(a, b) for a, b in zip(got.to_pylist(), want.to_pylist()) if a != b][:5])
    return rb


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, ROWS - 1, ROWS, ROWS + 1, 3 * ROWS + 5])
def test_row_counts_around_the_workgroup(gpu, n):
    t = shared_table(n)
    a = check(gpu, EVERY, t, srcs=uneven(t, [701, 13, 1500, 1]))
    b = check(gpu, EVERY, t, chunk=max(n, 1))
    for j in range(1, a.num_columns):
        assert raw_bytes(a.column(j)) == raw_bytes(b.column(j)), j


def _value(ln, seed):
    """A value of exactly `ln` bytes: words of 1- to 4-byte code points, delimiters and blanks, cut at a code point and filled with dots."""
    r = np.random.default_rng(seed)
    tokens = ["ab", " ", "é", "€", "\U0001F600", "/", "xyz", "  ", "//", "q"]
    out, size = [], 0
    while size < ln:
        tok = tokens[int(r.integers(0, len(tokens)))]
        if size + len(tok.encode()) > ln:
            tok = "." * (ln - size)
        out.append(tok)
        size += len(tok.encode())
    v = "".join(out)
    assert len(v.encode()) == ln
    return v


LONG_EXPRS = [split(c("s"), "/", 1), split(c("s"), "/", 3), split(c("s"), "/", 400), left(c("s"), 9), left(c("s"), 20_000), left(c("s"), -9), right(c("s"), 9), right(c("s"), 30_000),
              right(c("s"), -9), trim("btrim", c("s"), " ./"), trim("ltrim", c("s"), "ab /"), trim("rtrim", c("s")), split(c("s"), "//", 2), trim("btrim", c("s"), " é€/")]


@pytest.mark.gpu
def test_value_lengths_around_the_chunk_and_the_round(gpu):
    lengths = [0, 15, 16, 17, 70, ROUND - 1, ROUND, ROUND + 1, 3 * ROUND + 5]
    n = ROWS + 40
    s = [("r%d / x " % j) if j % 7 else None for j in range(n)]
    for j, ln in enumerate(lengths):
        s[5 + j * (n // len(lengths))] = _value(ln, ln)
    t = {"k": list(range(n)), "i": [j % 50 for j in range(n)], "s": s, "u": ["u"] * n}
    check(gpu, LONG_EXPRS, t, chunk=300)


@pytest.mark.gpu
def test_a_first_value_at_every_misalignment(gpu):
    """The batches are slices of one array that begin 0..15 bytes into its byte buffer (and the values behind start wherever the lengths put them)."""
    n = 400
    s = ["%s/é€ %d " % ("x" * (j % 16 == 0), j) for j in range(n)]
    s[:16] = ["m"] * 16                       # rows 0..15 are one byte each: a slice from row m starts m bytes into the buffer
    s[40], s[41] = None, ""
    t = {"k": list(range(n)), "i": [0] * n, "s": s, "u": [" u "] * n}
    whole = pa.record_batch([pa.array(t[cn], _PA[ty]) for cn, ty in COLS], names=[cn for cn, _ in COLS])
    exprs = [split(c("s"), "/", 2), left(c("s"), -3), right(c("s"), 4), trim("btrim", c("s"), "x 0123456789"), split(c("s"), "é€", 1), trim("rtrim", c("s"), " é0123456789")]
    for m in range(16):
        sub = {cn: v[m:] for cn, v in t.items()}
        assert np.frombuffer(whole.column(2).buffers()[1], dtype=np.int32)[m] == m
        check(gpu, exprs, sub, srcs=[whole.slice(m, 150), whole.slice(m + 150, n - m - 150)])


def _with_marks(ln, marks, mark, fill="a"):
    """`ln` bytes of `fill` with `mark` written at the given byte positions (inside the value)."""
    b = bytearray(fill.encode() * ln)[:ln]
    mb = mark.encode()
    for p in sorted(marks):
        if 0 <= p and p + len(mb) <= ln:
            b[p:p + len(mb)] = mb
    return b.decode()


@pytest.mark.gpu
def test_delimiters_at_the_ends_the_chunk_edges_and_the_round_edges(gpu):
    """One long value per group of rows, behind prefixes of 0..17 bytes, so that its delimiters fall on the last byte of a chunk, the first of the next,
    and on both sides of a round boundary whatever the buffer's own alignment; adjacent delimiters, a field that spans a round, n = the field count and
    one beyond."""
    ln = 2 * ROUND + 100
    marks = [0, 1, 15, 16, 17, 31, 32, 33, 34, 35, ROUND - 17, ROUND - 16, ROUND - 15, ROUND - 2, ROUND - 1, ROUND, ROUND + 1, ROUND + 15, ROUND + 16, ROUND + 17, 2 * ROUND - 1,
             2 * ROUND, 2 * ROUND + 16, ln - 2, ln - 1]
    long = _with_marks(ln, marks, "/")
    fields = len(marks) + 1
    assert long.count("/") == len(marks) and max(len(f) for f in long.split("/")) > ROUND - 100
    s = []
    for p in (0, 1, 2, 15, 16, 17):
        s += ["p" * p, long, None, "/", "a/", "/a", "//"]
    n = len(s)
    t = {"k": list(range(n)), "i": [0] * n, "s": s, "u": ["u"] * n}
    exprs = [split(c("s"), "/", j) for j in (1, 2, 3, 4, 5, 6, 10, 11, 12, 14, 15, 16, 17, 21, 22, fields - 2, fields - 1, fields, fields + 1)]
    exprs += [trim("btrim", c("s"), "/"), trim("ltrim", c("s"), "/a"), trim("rtrim", c("s"), "a/")]
    check(gpu, exprs, t, chunk=11)


@pytest.mark.gpu
def test_code_points_across_the_chunk_and_round_edges(gpu):
    """Values of 2-, 3- and 4-byte code points longer than a round, behind prefixes of 0..3 bytes: a code point lies across every chunk edge and across
    the round edge for some prefix; left / right with both signs, counts around the round boundary and around the value's length."""
    s = []
    for ch in ("é", "€", "\U0001F600"):
        w = len(ch.encode())
        cps = (ROUND + 200) // w
        for p in range(4):
            s += ["p" * p, ch * cps, None, ch, "a" + ch * 5 + "b"]
    n = len(s)
    t = {"k": list(range(n)), "i": [0] * n, "s": s, "u": ["u"] * n}
    counts = sorted({0, 1, 2, 5, 6, 7, 8, ROUND // 4 - 1, ROUND // 4, ROUND // 4 + 1, ROUND // 3, ROUND // 3 + 1, ROUND // 2 - 1, ROUND // 2, ROUND // 2 + 1,
                     (ROUND + 200) // 4 - 1, (ROUND + 200) // 4, (ROUND + 200) // 4 + 1, (ROUND + 200) // 3, (ROUND + 200) // 2 - 1, (ROUND + 200) // 2, (ROUND + 200) // 2 + 1})
    exprs = []
    for k in counts:
        exprs += [left(c("s"), k), right(c("s"), k)] + ([left(c("s"), -k), right(c("s"), -k)] if k else [])
    for a in range(0, len(exprs), 12):
        check(gpu, exprs[a:a + 12], t, chunk=9)


@pytest.mark.gpu
def test_trim_everything_nothing_and_across_a_round(gpu):
    blanks = " " * (ROUND + 300)
    s = []
    for p in (0, 1, 15, 16):
        s += ["p" * p, blanks, blanks + "x" + blanks, "x" + blanks, blanks + "x", "x", "", None, "  x y  ", "\t x \t", "xyx", " " * 15, " " * 16, " " * 17, "x" * 16 + " ", " " + "x" * 16]
    n = len(s)
    t = {"k": list(range(n)), "i": [0] * n, "s": s, "u": ["u"] * n}
    ascii_sets = [None, " ", " x", "xy \t", "", "p"]
    exprs = [trim(w, c("s"), cs) for w in ("ltrim", "rtrim", "btrim") for cs in ascii_sets]
    check(gpu, exprs, t, chunk=13)
    # the general kernel (a set with é / €) against the reference, and against the streaming kernel on these ASCII-only values
    general = [trim(w, c("s"), cs + "é€") for w in ("ltrim", "rtrim", "btrim") for cs in (" ", " x", "xy \t")]
    stream = [trim(w, c("s"), cs) for w in ("ltrim", "rtrim", "btrim") for cs in (" ", " x", "xy \t")]
    a, b = check(gpu, general, t, chunk=13), check(gpu, stream, t, chunk=13)
    for j in range(1, a.num_columns):
        assert raw_bytes(a.column(j)) == raw_bytes(b.column(j)), j
    # multi-byte characters to strip, on either side, beside bytes they share a prefix with
    m = ["é€xé€", "€", "éé€€", "xé", "èé x éè", "€₭€", None, "", " é ", "é" * 20_000 + "x" + "€" * 20_000]
    tm = {"k": list(range(len(m))), "i": [0] * len(m), "s": m, "u": ["u"] * len(m)}
    check(gpu, [trim(w, c("s"), cs) for w in ("ltrim", "rtrim", "btrim") for cs in ("é€", "é ", "€\U0001F600", "è")], tm)


@pytest.mark.gpu
def test_the_general_kernel_delimiters(gpu):
    d16 = "0123456789abcdef"
    s = ["aaaa", "aaa", "aa", "a", "", None, "xaay", "abcab", "a~@~b~@~~@~c", "€é1€é2€é€é", "é€é", d16, "x" + d16 + "y" + d16, d16[:15], d16 * 3, "ab" * 20_000 + "c" + "ab" * 5,
         "~@" * 9 + "~@~tail", "€" + "€é" * 3]
    n = len(s)
    t = {"k": list(range(n)), "i": [0] * n, "s": s, "u": ["u"] * n}
    exprs = [split(c("s"), d, k) for d in ("aa", "ab", "~@~", "€é", d16, "é€") for k in (1, 2, 3, 4)] + [split(c("s"), "ab", 20_001), split(c("s"), "ab", 20_002), split(c("s"), "ab", 20_007)]
    for a in range(0, len(exprs), 14):
        check(gpu, exprs[a:a + 14], t, chunk=5)
    # a one-byte delimiter on the streaming kernel and a two-byte one on the general kernel cut 'x/ /y' style values alike
    v = ["a/ b/ c", "/ ", "a", None, "/ / ", "x/ " * 3000]
    tv = {"k": list(range(len(v))), "i": [0] * len(v), "s": v, "u": ["u"] * len(v)}
    check(gpu, [trim("ltrim", split(c("s"), "/", 2)), split(c("s"), "/ ", 2), split(c("s"), "/ ", 3000), split(c("s"), "/ ", 3001), split(c("s"), "/ ", 3002)], tv)


@pytest.mark.gpu
def test_all_null_all_empty_and_a_tile_of_empty_slices(gpu):
    n = 3 * TILE + 7
    t = dict(shared_table(n))
    t["s"] = [None] * n
    rb = check(gpu, EVERY[:10], t)
    assert rb.column(1).null_count == n
    t["s"] = [""] * n
    rb = check(gpu, EVERY[:10] + EVERY[11:], t)
    assert rb.column(1).null_count == 0 and pc.sum(pc.binary_length(rb.column(1))).as_py() == 0
    # the second tile's slices are all empty -- no second field, nothing but blanks, fewer code points than are dropped -- between tiles that emit
    t["s"] = [("   " if TILE <= j < 2 * TILE else " a%d/b%d " % (j, j)) if j % 9 else None for j in range(n)]
    rb = check(gpu, [split(c("s"), "/", 2), trim("btrim", c("s")), left(c("s"), -3), right(c("s"), -3), split(c("s"), "a", 2), split(c("s"), "/b", 2)], t)
    for j in range(1, 7):
        assert pc.sum(pc.binary_length(rb.column(j).slice(TILE, TILE))).as_py() == 0 and pc.sum(pc.binary_length(rb.column(j).slice(0, TILE))).as_py() > 0


@pytest.mark.gpu
def test_nested_calls_and_slices_in_a_text_case(gpu):
    n = 2 * ROWS + 9
    t = dict(shared_table(n))
    t["s"] = [None if j % 13 == 0 else " k%d , x v%d x,, tail/%d " % (j, j, j) for j in range(n)]
    four = trim("rtrim", trim("ltrim", left(split(c("s"), ",", 2), 7)), "x ")
    exprs = [trim("btrim", split(c("s"), ",", 1)), trim("btrim", split(c("s"), ",", 2), " x"), four, right(trim("btrim", split(c("s"), ",", 4)), 3), left(right(c("s"), -2), -2),
             split(split(c("s"), ",", 2), " ", 3), trim("btrim", split(c("s"), " , ", 2), "xé "), left(split(c("s"), ",,", 2), -4), right(split(c("s"), "/", 2), 2)]
    check(gpu, exprs, t, srcs=uneven(t, [300, 7, 1100]))
    # THEN and ELSE beside a literal and a plain column; the same slice twice is one source
    e = case([(mod("i", 4, 0), split(c("s"), ",", 1)), (mod("i", 4, 1), lit_utf8("literal")), (mod("i", 4, 2), c("u")), (mod("i", 7, 3), split(c("s"), ",", 1)), (mod("i", 7, 4), lit_null())],
             trim("btrim", split(c("s"), ",", 2), " x"))
    no_else = case([(mod("i", 3, 0), left(c("u"), 4))])
    rb = check(gpu, [e, no_else, cast(four, "Utf8")], t)
    assert rb.column(1).null_count > 0 and rb.column(2).null_count > n // 2


def _rows(b):
    return list(zip(*[b.column(j).to_pylist() for j in range(b.num_columns)]))


@pytest.mark.gpu
def test_a_slice_as_group_by_order_by_distinct_and_count_distinct_key(gpu):
    from flock_amd.stages import StagedRun, build_query_dag
    n = 3 * ROWS + 5
    t = shared_table(n)
    key = split(c("u"), "/", 2)
    arg = trim("btrim", c("s"), " /")
    labels, args = ref.eval_text(key, t, TYPES), ref.eval_text(arg, t, TYPES)
    want = {}
    for lab, a in zip(labels, args):
        cnt, ca = want.get(lab, (0, 0))
        want[lab] = (cnt + 1, ca + (a is not None))
    want = sorted(((k, v[0], v[1]) for k, v in want.items()), key=repr)
    assert None in labels and len(want) > 5
    assert sorted(_rows(run(gpu, group_by(key, count_arg=arg), [(t, COLS)])), key=repr) == want
    # the staged run -- the plan cut at its repartition by the splitter -- equals the whole plan
    dag = build_query_dag(group_by(key, parts=4, count_arg=arg))
    assert len(dag) == 2
    staged = StagedRun(gpu, dag, instances=1, on_device=True)
    try:
        out = staged.run({"events": batches(t, n)[0]})
    finally:
        staged.close()
    out = out if isinstance(out, list) else [out]
    assert sorted([r for b in out for r in _rows(b)], key=repr) == want
    # ORDER BY right(s, 3) [DESC], k: NULL keys last
    okey = right(c("s"), 3)
    ol = ref.eval_text(okey, t, TYPES)
    for desc in (False, True):
        rb = run(gpu, projection([(c("k"), "k")], sort_(scan(), [(okey, desc), (c("k"), False)])), [(t, COLS)])
        some = sorted((j for j in range(n) if ol[j] is not None), key=lambda j: (ol[j].encode(), j))
        if desc:
            some = sorted((j for j in range(n) if ol[j] is not None), key=lambda j: ([-b for b in ol[j].encode()] + [1], j))
        assert rb.column(0).to_pylist() == some + [j for j in range(n) if ol[j] is None], desc
    # DISTINCT left(s, 2); COUNT(DISTINCT btrim(s, ' /')), COUNT(*)
    dl = ref.eval_text(left(c("s"), 2), t, TYPES)
    assert sorted(run(gpu, distinct(left(c("s"), 2)), [(t, COLS)]).column(0).to_pylist(), key=repr) == sorted(set(dl), key=repr)
    assert _rows(run(gpu, count_distinct(arg), [(t, COLS)])) == [(len({v for v in args if v is not None}), n)]


@pytest.mark.gpu
def test_over_a_filter_under_joins_and_under_sort_and_limit(gpu):
    n = 2 * ROWS + 11
    t = shared_table(n)
    e = trim("btrim", split(c("u"), "/", 1))
    pred = binary(binary(c("i"), "Gt", lit("Int32", 50)), "And", binary(c("k"), "Lt", lit("Int32", n - 100)))
    keep = sref.eval_rows(pred, t, TYPES, want="Boolean")
    kept = {name: [v for v, b in zip(col, keep) if b is True] for name, col in t.items()}
    assert 0 < len(kept["k"]) < n
    rb = run(gpu, projection([(c("k"), "k"), (e, "x"), (right(c("s"), 2), "y")], filter_(pred)), [(t, COLS)])
    assert rb.column(0).to_pylist() == kept["k"] and rb.column(1).equals(pa.array(ref.eval_text(e, kept, TYPES), pa.string()))
    assert rb.column(2).equals(pa.array(ref.eval_text(right(c("s"), 2), kept, TYPES), pa.string()))
    # the projection BELOW the join: its slice is a column the join carries
    below = [("k", "Int32"), ("i", "Int32"), ("x", "Utf8")]
    lproj = projection([(c("k"), "k"), (c("i"), "i"), (e, "x")])
    x = ref.eval_text(e, t, TYPES)
    rcols = [("name", "Utf8"), ("w", "Int32")]
    right_t = {"name": ["u%d" % j for j in range(0, 50, 3)] + [None, ""], "w": list(range(19))}
    semi = {"execution_plan": "hash_join_exec", "left": lproj, "right": scan(rcols), "join_type": "Semi", "mode": "CollectLeft", "on": [[c("i", below), c("w", rcols)]],
            "schema": {"fields": [_field(nm, ty) for nm, ty in below], "metadata": {}}}
    rb = run(gpu, semi, [(t, COLS), (right_t, rcols)])
    rows = [j for j in range(n) if t["i"][j] is not None and 0 <= t["i"][j] < 19]
    assert sorted(_rows(rb), key=repr) == sorted(((t["k"][j], t["i"][j], x[j]) for j in rows), key=repr) and len(rows) > 50
    inner = {"execution_plan": "hash_join_exec", "left": lproj, "right": scan(rcols), "join_type": "Inner", "mode": "CollectLeft", "on": [[c("i", below), c("w", rcols)]],
             "schema": {"fields": [_field(nm, ty) for nm, ty in below + rcols], "metadata": {}}}
    rb = run(gpu, inner, [(t, COLS), (right_t, rcols)])
    want = [(t["k"][j], t["i"][j], x[j], right_t["name"][t["i"][j]], t["i"][j]) for j in range(n) if t["i"][j] is not None and 0 <= t["i"][j] < 19]
    assert sorted(_rows(rb), key=repr) == sorted(want, key=repr) and len(want) > 50
    # under a sort + limit: the projection below them
    lim = {"execution_plan": "global_limit_exec", "limit": 40, "input": sort_(lproj, [(c("k", below), True)])}
    rb = run(gpu, lim, [(t, COLS)])
    assert _rows(rb) == [(t["k"][j], t["i"][j], x[j]) for j in range(n - 1, n - 41, -1)]


@pytest.mark.gpu
def test_both_fixtures_end_to_end(gpu):
    n = 5000
    r = np.random.default_rng(22)
    dirs = ["", "a", "item", "é€", "deep"]
    url = [None if j % 17 == 0 else "https://www.nexmark.com/%s/%s/item.htm?query=%d" % (dirs[int(r.integers(0, 5))], dirs[int(r.integers(0, 5))], j) if j % 5 else "http://x/%d" % j
           for j in range(n)]
    bid_cols = [("auction", "Int32"), ("bidder", "Int32"), ("price", "Int32"), ("url", "Utf8")]
    bid = {"auction": list(range(n)), "bidder": [j % 7 for j in range(n)], "price": [j * 3 for j in range(n)], "url": url}
    rb = run(gpu, open(os.path.join(PLANS, "q22_url_dirs.json")).read(), [(bid, bid_cols)], chunk=1700)
    assert rb.schema.names == ["auction", "bidder", "price", "dir1", "dir2"]
    want = [(a, b, p, None if u is None else ref.split_part(u, "/", 4), None if u is None else ref.split_part(u, "/", 5)) for a, b, p, u in zip(bid["auction"], bid["bidder"], bid["price"], url)]
    assert _rows(rb) == want and {w[3] for w in want} >= {None, "", "a", "é€"}
    mail = [None if j % 19 == 0 else "user%d@%s" % (j, ["example.com", "nexmark.org", "é.example", ""][j % 4]) if j % 11 else "no-at-sign-%d" % j for j in range(n)]
    rb = run(gpu, open(os.path.join(PLANS, "person_email_domains.json")).read(), [({"email_address": mail}, [("email_address", "Utf8")])], chunk=1700)
    counts = {}
    for m in mail:
        d = None if m is None else ref.split_part(m, "@", 2)
        counts[d] = counts.get(d, 0) + 1
    assert rb.schema.names == ["domain", "COUNT(UInt8(1))"] and sorted(_rows(rb), key=repr) == sorted(counts.items(), key=repr) and len(counts) == 5


@pytest.mark.gpu
def test_execute_twice_and_in_other_batch_sizes(gpu):
    from flock_amd.runtime import ExecutionContext
    exprs = EVERY + [trim("btrim", split(c("s"), "/", 2)), case([(mod("i", 2, 0), left(c("s"), 2))], right(c("u"), 3))]
    plan = projection([(c("k"), "k")] + [(e, "x%d" % j) for j, e in enumerate(exprs)])
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        for n in (2 * ROWS + 3, 2 * ROWS + 3, ROWS - 1, 1):
            t = shared_table(n)
            want = [pa.array(ref.eval_text(e, t, TYPES), pa.string()) for e in exprs]
            seen = []
            for sizes in ([3000], [257, 1024, 5], [1]) if n > 1 else ([1],):
                if sizes == [1] and n > 1:
                    sizes = [n]
                ctx.feed_data_sources([[uneven(t, sizes)]])
                for _ in range(2):
                    rb = ctx.execute()[0][0]
                    assert rb.num_rows == n
                    for j, w in enumerate(want):
                        assert rb.column(1 + j).equals(w), (n, sizes, j)
                    seen.append([raw_bytes(rb.column(1 + j)) for j in range(len(exprs))])
                ctx.clean_data_sources()
            assert all(s == seen[0] for s in seen[1:])
    finally:
        ctx.close()
