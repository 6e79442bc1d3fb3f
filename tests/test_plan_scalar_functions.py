"""Scalar functions in expressions (flock_amd/csrc/valprog.hpp A-F1..A-F8): abs / signum / floor / ceil / round / trunc / sqrt over Float64, date_trunc /
date_part over Timestamp(ms), octet_length / char_length over Utf8, now() -- in projections, filters, under CASE / arithmetic / IN / IS NULL, as GROUP BY
and ORDER BY keys, under joins and in stage plans.  Every comparison is row for row and in order against tests/scalar_fn_ref.py, Float64 as bit patterns."""
import ctypes as C
import json
import math
import os
import subprocess
import time

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import scalar_fn_ref as ref
from oracle import generic_ops as g
from scalar_fn_ref import TS, fn, lit_utf8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")

COLS = [("k", "Int32"), ("i", "Int32"), ("l", "Int64"), ("f", "Float64"), ("t", "ts"), ("s", "Utf8")]
NAMES = [c for c, _ in COLS]
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string(), "ts": pa.timestamp("ms")}
TYPES = {c: (TS if t == "ts" else t) for c, t in COLS}
SIZES = [1, 8193, 20_011]            # one row; one full flag tile plus one row; two tiles plus a ragged one
SPECIAL_F = [0.0, -0.0, 0.5, -0.5, 1.5, 2.5, -2.5, 0.49999999999999994, -0.49999999999999994, math.nan, math.inf, -math.inf, 4.0, 2.0, 1e300, 5e-324, -7.25,
             4503599627370495.5, 4503599627370496.0, -4503599627370497.0, 9007199254740993.0]
SPECIAL_T = [-1, 0, 1436918400123, 951782400000, 951868799999, -2203891200000, -2203891200001, 4107456000000, 4107542399999, 1, -86_400_001, 1704067199999, 1704067200000]
TEXT = ["", "a", "été", "€", "\U0001F600", "aé€\U0001F600", "w" * 70, "é" * 35, "x" * 15 + "€", "x" * 14 + "\U0001F600" + "yz"]
MATH = list(ref.MATH)


def _dt(t):
    return TS if t == "ts" else t


def _field(name, t, nullable=True):
    return {"data_type": _dt(t), "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


def c(name, cols=COLS):
    return {"physical_expr": "column", "name": name, "index": [n for n, _ in cols].index(name)}


def lit(kind, v):
    return {"physical_expr": "literal", "value": {kind: v}}


def binary(l, op, r):
    return {"physical_expr": "binary_expr", "left": l, "op": op, "right": r}


def unary(tag, arg):
    return {"physical_expr": tag, "arg": arg}


def cast(e, t):
    return {"physical_expr": "cast_expr", "expr": e, "cast_type": t}


def case(whens, els=None):
    return {"physical_expr": "case_expr", "expr": None, "when_then_expr": [[w, t] for w, t in whens], "else_expr": els}


def trunc(unit, e=None):
    return fn("date_trunc", lit_utf8(unit), c("t") if e is None else e)


def part(unit, e=None):
    return fn("date_part", lit_utf8(unit), c("t") if e is None else e)


def scan(cols=COLS):
    return {"execution_plan": "memory_exec", "schema": {"fields": [_field(n, t) for n, t in cols], "metadata": {}}, "projection": list(range(len(cols)))}


def out_type(e, types=TYPES):
    """The serialised data_type of an expression's column."""
    if e.get("physical_expr") == "scalar_function_expr":
        return ref.result_type(e.get("name") or e.get("fun") or "abs")
    if e.get("physical_expr") == "column":
        return types[e["name"]]
    x, _, ty = ref.rewrite(e, {n: [] for n in types}, types)
    return g.static_type(x, ty) or "Int64"


def projection(exprs, inp=None, types=TYPES):
    return {"execution_plan": "projection_exec", "expr": [[e, n] for e, n in exprs], "input": scan() if inp is None else inp,
            "schema": {"fields": [_field(n, "x") | {"data_type": out_type(e, types)} for e, n in exprs], "metadata": {}}}


def filter_(pred, inp=None):
    return {"execution_plan": "filter_exec", "predicate": pred, "input": scan() if inp is None else inp}


def make_table(n, seed, null_p=0.15):
    r = np.random.default_rng(seed)
    nul = lambda xs: [None if r.random() < null_p else x for x in xs]
    f = [float(x) for x in np.round(r.normal(0, 50, n), 2)]
    t = [int(x) for x in r.integers(-2_300_000_000_000, 4_200_000_000_000, n)]        # 1897 .. 2103
    for j in range(n):                                                                   # the special values, spread over the rows
        if j % 3 == 0:
            f[j] = SPECIAL_F[(j // 3) % len(SPECIAL_F)]
        if j % 4 == 1:
            t[j] = SPECIAL_T[(j // 4) % len(SPECIAL_T)]
    return {"k": list(range(n)), "i": nul([int(x) for x in r.integers(-40, 400, n)]), "l": nul([int(x) for x in r.integers(-2**40, 2**40, n)]), "f": nul(f), "t": nul(t),
            "s": nul([TEXT[int(x)] + ("%d" % x if x % 3 == 0 else "") for x in r.integers(0, len(TEXT), n)])}


def batches(t, chunk, cols=COLS):
    n = len(t[cols[0][0]])
    return [pa.record_batch([pa.array(t[cn][a:a + chunk], _PA[ty]) for cn, ty in cols], names=[cn for cn, _ in cols]) for a in range(0, max(n, 1), max(chunk, 1))]


def pyrows(rb):
    cols = []
    for i in range(rb.num_columns):
        col = rb.column(i)
        if pa.types.is_timestamp(col.type):
            col = col.cast(pa.int64())
        vals = col.to_pylist()
        if pa.types.is_floating(col.type):
            vals = [ref.bits(v) for v in vals]
        cols.append(vals)
    return list(zip(*cols)) if cols else []


def want_rows(cols):
    return list(zip(*[[ref.bits(v) if isinstance(v, float) else v for v in col] for col in cols])) if cols else []


def refused(plan, *words):
    from flock_amd import _ffi
    from flock_amd.runtime import FlockGpuError, explain
    with pytest.raises(FlockGpuError) as e:
        explain(plan)
    assert e.value.code == _ffi.ERR_UNSUPPORTED, str(e.value)
    for w in ("scalar_function_expr",) + words:
        assert w in str(e.value), (w, str(e.value))


# ------------------------------------------------------------------ CPU: the reference on hand-worked rows
def test_reference_math_by_hand():
    b = ref.bits
    rows = {"round": [(0.5, 1.0), (-0.5, -1.0), (2.5, 3.0), (-2.5, -3.0), (1.5, 2.0), (0.49999999999999994, 0.0), (-0.4, -0.0), (-0.0, -0.0), (math.inf, math.inf),
                      (4503599627370495.5, 4503599627370496.0), (9007199254740993.0, 9007199254740992.0)],
            "signum": [(0.0, 1.0), (-0.0, -1.0), (math.inf, 1.0), (-math.inf, -1.0), (-3.5, -1.0), (5e-324, 1.0)],
            "abs": [(-0.0, 0.0), (-math.inf, math.inf), (-7.25, 7.25), (3.0, 3.0)],
            "floor": [(-0.0, -0.0), (0.5, 0.0), (-0.5, -1.0), (2.5, 2.0), (-2.5, -3.0), (-math.inf, -math.inf), (1e300, 1e300)],
            "ceil": [(-0.5, -0.0), (0.5, 1.0), (-0.0, -0.0), (0.0, 0.0), (2.5, 3.0), (-2.5, -2.0)],
            "trunc": [(-0.5, -0.0), (0.5, 0.0), (2.5, 2.0), (-2.5, -2.0), (-0.0, -0.0), (math.inf, math.inf)],
            "sqrt": [(4.0, 2.0), (-0.0, -0.0), (0.0, 0.0), (2.0, 1.4142135623730951), (math.inf, math.inf), (1e300, 1e150)]}
    for name, pairs in rows.items():
        for x, y in pairs:
            assert b(ref.call(name, [x])) == b(y), (name, x, ref.call(name, [x]), y)
        assert b(ref.call(name, [math.nan])) == "nan" and ref.call(name, [None]) is None
    assert b(ref.call("sqrt", [-1.0])) == "nan" and b(ref.call("sqrt", [-math.inf])) == "nan"


def test_signum_is_not_arrows_sign_at_zero():
    """Rust's f64::signum gives +-1.0 at +-0.0; Arrow's `sign` gives a zero there.  They differ by design: the library follows Rust (A-F3)."""
    got = pc.sign(pa.array([0.0, -0.0, 3.0, -math.inf])).to_pylist()
    assert got[:2] == [0.0, 0.0]
    assert [ref.fn_signum(v) for v in (0.0, -0.0)] == [1.0, -1.0]
    assert got[2:] == [ref.fn_signum(3.0), ref.fn_signum(-math.inf)]


def test_reference_time_by_hand():
    D = ref.MS_DAY
    assert ref.date_trunc("day", -1) == -D and ref.date_trunc("second", -1) == -1000 and ref.date_trunc("year", -1) == -365 * D
    assert ref.date_trunc("week", 0) == -3 * D and ref.date_trunc("WEEK", 4 * D) == 4 * D            # 1970-01-05 was a Monday
    assert [ref.date_part(u, -1) for u in ref.PART_UNITS] == [1969, 12, 31, 23, 59, 59, 3, 365]
    assert [ref.date_part(u, 0) for u in ref.PART_UNITS] == [1970, 1, 1, 0, 0, 0, 4, 1]
    t = 1436918400123                                                                                  # 2015-07-15T00:00:00.123, a Wednesday
    assert [ref.date_part(u, t) for u in ref.PART_UNITS] == [2015, 7, 15, 0, 0, 0, 3, 196]
    assert ref.date_trunc("minute", t) == 1436918400000 and ref.date_trunc("month", t) == 1435708800000 and ref.date_trunc("year", t) == 1420070400000
    leap = 951782400000                                                                                # 2000-02-29
    assert [ref.date_part(u, leap) for u in ("year", "month", "day", "doy", "dow")] == [2000, 2, 29, 60, 2]
    assert ref.date_trunc("month", leap) == leap - 28 * D and ref.date_part("day", leap + D) == 1
    m1900 = -2203891200000                                                                             # 1900-03-01: 1900 is no leap year
    assert [ref.date_part(u, m1900) for u in ("year", "month", "day", "doy")] == [1900, 3, 1, 60]
    assert [ref.date_part(u, m1900 - 1) for u in ("month", "day", "hour", "second")] == [2, 28, 23, 59]
    f2100 = 4107456000000                                                                              # 2100-02-28; the next day is 1 March
    assert [ref.date_part(u, f2100) for u in ("year", "month", "day")] == [2100, 2, 28] and [ref.date_part(u, f2100 + D) for u in ("month", "day", "doy")] == [3, 1, 60]
    assert ref.call("date_trunc", ["day", None]) is None and ref.call("date_part", ["hour", None]) is None


def test_reference_text_by_hand():
    for s, chars, octets in (("", 0, 0), ("été", 3, 5), ("€", 1, 3), ("\U0001F600", 1, 4), ("aé€\U0001F600", 4, 10)):
        assert ref.char_length(s) == chars and ref.octet_length(s) == octets, s
    assert ref.call("length", ["été"]) == 3 and ref.call("character_length", ["€"]) == 1 and ref.call("octet_length", [None]) is None


@pytest.mark.parametrize("seed", range(3))
def test_reference_against_pyarrow(seed):
    r = np.random.default_rng(40 + seed)
    n = 3000
    mask = r.random(n) < 0.15
    ts = np.concatenate([r.integers(-2_300_000_000_000, 4_200_000_000_000, n - len(SPECIAL_T)), np.array(SPECIAL_T)])
    ta = pa.array(ts, pa.int64(), mask=mask).cast(pa.timestamp("ms"))
    tv = [None if m else int(x) for x, m in zip(ts, mask)]
    for u in ref.TRUNC_UNITS:
        got = pc.floor_temporal(ta, unit=u, week_starts_monday=True).cast(pa.int64()).to_pylist()
        assert got == [ref.call("date_trunc", [u, v]) for v in tv], u
    arrow = {"year": pc.year, "month": pc.month, "day": pc.day, "hour": pc.hour, "minute": pc.minute, "second": pc.second,
             "dow": lambda a: pc.day_of_week(a, count_from_zero=True, week_start=7), "doy": pc.day_of_year}
    for u in ref.PART_UNITS:
        assert arrow[u](ta).to_pylist() == [ref.call("date_part", [u, v]) for v in tv], u
    fs = np.concatenate([np.round(r.normal(0, 1000, n - len(SPECIAL_F)), 1) / 2, np.array(SPECIAL_F)])
    fa = pa.array(fs, pa.float64(), mask=mask)
    fv = [None if m else float(x) for x, m in zip(fs, mask)]
    arrow = {"abs": pc.abs, "floor": pc.floor, "ceil": pc.ceil, "trunc": pc.trunc, "sqrt": pc.sqrt, "round": lambda a: pc.round(a, round_mode="half_towards_infinity")}
    # (Arrow's round adds a half and floors: at the neighbours of +-0.5 below it in magnitude it answers +-1.0 where Rust's f64::round -- and the reference --
    # answer +-0.0; test_reference_math_by_hand pins those two)
    skip = {0.49999999999999994, -0.49999999999999994}
    for name, f in arrow.items():
        got = f(fa).to_pylist()
        for v, have in zip(fv, got):
            if not (name == "round" and v in skip):
                assert ref.bits(have) == ref.bits(ref.call(name, [v])), (name, v)
    words = [None if m else TEXT[int(x)] for x, m in zip(r.integers(0, len(TEXT), 200), mask)]
    sa = pa.array(words, pa.string())
    assert pc.utf8_length(sa).to_pylist() == [ref.call("char_length", [w]) for w in words]
    assert pc.binary_length(sa).to_pylist() == [ref.call("octet_length", [w]) for w in words]


def test_calendar_header_on_the_cpu():
    """flock_amd/csrc/calendar.hpp with g++: every day of 1600..2400 against a from-scratch day count, every unit, the round trip."""
    exe = os.path.join(ROOT, "tests", "cpp", "calendar_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "flock_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "calendar_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok 292560"), out.stdout + out.stderr


# ------------------------------------------------------------------ CPU: parsing, explain, refusals
def test_explain_shows_the_functions():
    from flock_amd.runtime import explain
    txt = explain(filter_(binary(fn("abs", c("f")), "Gt", lit("Float64", 3.0))))
    assert txt.splitlines()[0].startswith("Filter(abs(f) > 3)"), txt
    txt = explain(projection([(c("k"), "k"), (trunc("day"), "d"), (fn("now"), "p_time"), (part("hour"), "h"), (fn("char_length", c("s")), "n"), (fn("SQRT", c("f")), "r")]))
    first = txt.splitlines()[0]
    assert first.startswith("Project(d = date_trunc('day', t), p_time = now(), h = date_part('hour', t), n = char_length(s), r = sqrt(f)) ["), txt
    assert "d:Timestamp(ms)" in first and "p_time:Timestamp(ms)" in first and "h:Int32" in first and "n:Int32" in first and "r:Float64" in first, txt
    # `fun` for `name`, any letter case, the aliases of char_length, a unit in capitals, no return_type
    alias = {"physical_expr": "scalar_function_expr", "fun": "Character_Length", "args": [cast(c("s"), "Utf8")]}
    up = {"physical_expr": "scalar_function_expr", "name": "DATE_TRUNC", "args": [lit_utf8("MONTH"), trunc("day")]}
    txt = explain(projection([(alias, "n"), (fn("length", c("s")), "m"), (up, "mo")]))
    assert "n = char_length(s), m = char_length(s), mo = date_trunc('month', date_trunc('day', t))" in txt and "mo:Timestamp(ms)" in txt, txt
    # under CASE, arithmetic, IN and IS NULL
    e = case([(unary("is_null_expr", part("dow")), lit("Float64", 0.0))], binary(fn("floor", c("f")), "Multiply", lit("Float64", 2.0)))
    assert "Project(x = CASE ...)" in explain(projection([(e, "x")]))
    inl = {"physical_expr": "in_list_expr", "expr": part("dow"), "negated": False, "list": [lit("Int32", 0), lit("Int32", 6)]}
    assert "Filter(date_part('dow', t) IN (0, 6))" in explain(filter_(inl))


def test_refusals_name_their_cause():
    one = lambda e: projection([(e, "x")])
    for name in ("exp", "ln", "log", "log2", "log10", "power", "sin", "cos", "tan", "asin", "acos", "atan"):
        refused(one(fn(name, c("f"))), "'" + name + "'", "no bit-exact counterpart on the device")
    for name in ("substr", "lower", "upper", "trim", "concat"):
        refused(one(fn(name, c("s"))), "'" + name + "'", "not yet")
    refused(one(fn("starts_with", c("s"), lit_utf8("a"))), "starts_with", "Boolean")
    refused(one(fn("frobnicate", c("f"))), "'frobnicate'")
    refused(one({"physical_expr": "scalar_function_expr"}), "function name")
    for name in MATH:
        refused(one(fn(name, c("i"))), "'" + name + "'", "Int32", "integer argument")
        refused(one(fn(name, c("l"))), "'" + name + "'", "Int64", "integer argument")
        refused(one(fn(name, c("t"))), "'" + name + "'", "Timestamp")
    refused(one(fn("round", c("f"), lit("Int64", 2))), "'round'", "2 arguments")
    refused(one(fn("abs")), "'abs'", "0 arguments")
    for f, good in (("date_trunc", "second, minute, hour, day, week, month, year"), ("date_part", "year, month, day, hour, minute, second, dow, doy")):
        refused(one(fn(f, lit_utf8("fortnight"), c("t"))), f, "unit 'fortnight'", good)
        refused(one(fn(f, c("s"), c("t"))), f, "unit", "Utf8 literal")
        refused(one(fn(f, lit("Int64", 3), c("t"))), f, "unit", "Utf8 literal")
        refused(one(fn(f, lit_utf8("day"), c("l"))), f, "Int64", "Timestamp")
        refused(one(fn(f, lit_utf8("day"), part("hour"))), f, "Int32", "Timestamp")
        refused(one(fn(f, lit_utf8("day"))), f, "1 arguments")
    refused(one(trunc("dow")), "date_trunc", "unit 'dow'")
    refused(one(part("week")), "date_part", "unit 'week'")
    for f in ("octet_length", "char_length", "length", "character_length"):
        refused(one(fn(f, c("i"))), "Utf8 column", "Int32")
        refused(one(fn(f, lit_utf8("abc"))), "Utf8 column")
        refused(one(fn(f, c("s"), c("s"))), "2 arguments")
    refused(one(fn("now", c("t"))), "'now'", "1 arguments")
    for e, ty, what in ((fn("abs", c("f")), "Int64", "Float64"), (trunc("day"), "Int64", "Timestamp(ms)"), (part("day"), "Int64", "Int32"), (fn("now"), "Float64", "Timestamp(ms)"),
                        (fn("char_length", c("s")), TS, "Int32")):
        bad = dict(e, return_type=ty)
        refused(one(bad), "return_type", what)
    # in a predicate, a GROUP BY key and an ORDER BY key the refusal is the same one
    refused(filter_(binary(fn("exp", c("f")), "Gt", lit("Float64", 1.0))), "'exp'")
    refused({"execution_plan": "sort_exec", "input": scan(), "expr": [{"expr": fn("lower", c("s")), "options": {"descending": False, "nulls_first": False}}]}, "'lower'")
    # what stays refused: a Boolean projection, hash partitioning on a computed expression
    from flock_amd.runtime import FlockGpuError, explain
    with pytest.raises(FlockGpuError) as e:
        explain(projection([(binary(fn("abs", c("f")), "Gt", lit("Float64", 1.0)), "b")]))
    assert "Boolean" in str(e.value)
    with pytest.raises(FlockGpuError) as e:
        explain({"execution_plan": "repartition_exec", "input": scan(), "partitioning": {"Hash": [[trunc("minute")], 4]}})
    assert "Hash partitioning on a computed expression" in str(e.value)


def _group_by_minute(parts=None):
    """SELECT date_trunc('minute', t), COUNT(*), MAX(i) GROUP BY 1 -- Partial / [Hash] / Final."""
    aggs = [{"aggregate_expr": "count", "name": "COUNT(UInt8(1))", "data_type": "UInt64", "nullable": True, "expr": lit("UInt8", 1)},
            {"aggregate_expr": "max", "name": "MAX(i)", "data_type": "Int32", "nullable": True, "expr": c("i")}]
    key = "datetrunc(Utf8(\"minute\"),t)"
    partial = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [[trunc("minute"), key]], "aggr_expr": aggs, "input": scan(),
               "schema": {"fields": [_field(key, "ts"), _field("COUNT(UInt8(1))[count]", "UInt64"), _field("MAX(i)[max]", "Int32")], "metadata": {}},
               "input_schema": {"fields": [_field(n, t) for n, t in COLS], "metadata": {}}}
    mid = partial
    if parts:
        mid = {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096,
               "input": {"execution_plan": "repartition_exec", "input": partial, "partitioning": {"Hash": [[{"physical_expr": "column", "name": key, "index": 0}], parts]}}}
    return {"execution_plan": "hash_aggregate_exec", "mode": "FinalPartitioned" if parts else "Final", "group_expr": [[{"physical_expr": "column", "name": key, "index": 0}, key]],
            "aggr_expr": aggs, "input": mid,
            "schema": {"fields": [_field(key, "ts"), _field("COUNT(UInt8(1))", "UInt64"), _field("MAX(i)", "Int32")], "metadata": {}},
            "input_schema": {"fields": [_field(n, t) for n, t in COLS], "metadata": {}}}


def test_new_fixtures_parse_and_a_q2_look_alike_is_not_fused():
    from flock_amd import _ffi, build
    from flock_amd.runtime import explain
    txt = explain(open(os.path.join(PLANS, "q12_p_time.json")).read())
    assert txt.splitlines()[0].startswith("Project(p_time = now()) [") and "p_time:Timestamp(ms)" in txt.splitlines()[0] and "Scan(bid)" in txt, txt
    txt = explain(open(os.path.join(PLANS, "q12.json")).read())
    assert txt.splitlines()[0] == "Project [bidder:Int32, bid_count:UInt64, start_time:Timestamp(ms), end_time:Timestamp(ms)]" and "Aggregate(Partial)" in txt, txt
    build.build()
    lib = _ffi.load()
    got = C.c_int(-1)
    q2 = open(os.path.join(PLANS, "q2.json")).read().encode()
    assert lib.flockgpu_plan_recognise(q2, len(q2), C.byref(got)) == _ffi.OK and got.value == 2

    def with_function(node):          # the first `% 123 = 0` predicate found: its left side wrapped as CAST(abs(CAST(x AS Float64)) AS Int64)
        if isinstance(node, dict):
            if node.get("execution_plan") == "filter_exec":
                p = node["predicate"]
                p["left"] = cast(fn("abs", cast(p["left"], "Float64")), "Int64")
                return True
            return any(with_function(v) for v in node.values())
        if isinstance(node, list):
            return any(with_function(v) for v in node)
        return False
    plan = json.loads(q2)
    assert with_function(plan)
    text = json.dumps(plan).encode()
    assert lib.flockgpu_plan_recognise(text, len(text), C.byref(got)) == _ffi.OK and got.value == 0
    assert "fused" not in explain(plan) and "abs(" in explain(plan)


def test_a_group_by_date_trunc_plan_splits_into_stages_that_each_explain():
    from flock_amd.runtime import explain
    from flock_amd.stages import build_query_dag
    whole = explain(_group_by_minute(parts=4))
    assert "date_trunc('minute', t)" in whole, whole
    stages = build_query_dag(_group_by_minute(parts=4))
    assert len(stages) == 2 and stages[0].is_shuffling
    texts = [explain(st.plan) for st in stages]
    assert "date_trunc('minute', t)" in texts[0] and "Aggregate(Partial)" in texts[0] and "Aggregate(FinalPartitioned)" in texts[1], texts
    assert ":Timestamp(ms)" in texts[1].splitlines()[0]


def _rand_fvalue(r, depth):
    """A Float64-valued tree that mixes functions with arithmetic and CASE."""
    k = r.random()
    if depth == 0 or k < 0.15:
        return c("f") if r.random() < 0.7 else lit("Float64", float(r.choice([0.5, -2.0, 3.25, 10.0])))
    if k < 0.5:
        return fn(str(r.choice(MATH)), _rand_fvalue(r, depth - 1))
    if k < 0.7:
        return binary(_rand_fvalue(r, depth - 1), str(r.choice(["Plus", "Minus", "Multiply"])), _rand_fvalue(r, depth - 1))
    if k < 0.8:
        return cast(_rand_ivalue(r, depth - 1), "Float64")
    return case([(_rand_bool(r, depth - 1), _rand_fvalue(r, depth - 1))], _rand_fvalue(r, depth - 1) if r.random() < 0.6 else None)


def _rand_ivalue(r, depth):
    """An Int32-valued tree: date_part, the text lengths, Int32 columns, arithmetic on them."""
    k = r.random()
    if depth == 0 or k < 0.15:
        return c("i") if r.random() < 0.7 else lit("Int32", int(r.choice([1, -1, 7, 30, 100])))
    if k < 0.45:
        t = c("t") if r.random() < 0.6 else trunc(str(r.choice(ref.TRUNC_UNITS)))
        return part(str(r.choice(ref.PART_UNITS)), t)
    if k < 0.6:
        return fn(str(r.choice(["char_length", "octet_length"])), c("s"))
    if k < 0.8:
        return binary(_rand_ivalue(r, depth - 1), str(r.choice(["Plus", "Minus", "Multiply"])), _rand_ivalue(r, depth - 1))
    return case([(_rand_bool(r, depth - 1), _rand_ivalue(r, depth - 1))], _rand_ivalue(r, depth - 1) if r.random() < 0.6 else None)


def _rand_tvalue(r, depth):
    return trunc(str(r.choice(ref.TRUNC_UNITS)), c("t") if depth == 0 or r.random() < 0.6 else _rand_tvalue(r, depth - 1))


def _rand_bool(r, depth):
    k = r.random()
    cmp = str(r.choice(["Eq", "NotEq", "Lt", "LtEq", "Gt", "GtEq"]))
    if depth == 0 or k < 0.3:
        return binary(_rand_fvalue(r, max(depth - 1, 0)), cmp, _rand_fvalue(r, max(depth - 1, 0)))
    if k < 0.5:
        return binary(_rand_ivalue(r, depth - 1), cmp, _rand_ivalue(r, depth - 1))
    if k < 0.6:
        return binary(_rand_tvalue(r, depth - 1), cmp, c("t"))
    if k < 0.7:
        which = r.random()
        return unary("is_null_expr" if r.random() < 0.5 else "is_not_null_expr", _rand_fvalue(r, depth - 1) if which < 0.4 else _rand_ivalue(r, depth - 1) if which < 0.8 else _rand_tvalue(r, depth - 1))
    if k < 0.8:
        return {"physical_expr": "in_list_expr", "expr": _rand_ivalue(r, depth - 1), "negated": bool(r.random() < 0.4),
                "list": [lit("Int32", int(x)) for x in r.integers(0, 60, int(r.integers(1, 4)))]}
    if k < 0.85:
        return unary("not_expr", _rand_bool(r, depth - 1))
    return binary(_rand_bool(r, depth - 1), "And" if k < 0.93 else "Or", _rand_bool(r, depth - 1))


TREE_DEPTH = 3


def _trees(seed):
    """The three (projection expressions, predicate) pairs of a seed."""
    r = np.random.default_rng(9100 + seed)
    out = []
    for _ in range(3):
        exprs = [(c("k"), "k"), (_rand_fvalue(r, TREE_DEPTH), "x"), (_rand_ivalue(r, TREE_DEPTH), "y"), (_rand_tvalue(r, 2), "z")]
        out.append((exprs, _rand_bool(r, TREE_DEPTH)))
    return out


def _program_size(e):
    """Upper bounds of what the expression costs one program of the evaluator: (operators, distinct columns) -- every node at most one operator, an
    IN item three (operand again, compare, OR), a CASE branch one more (Select)."""
    cols = set()

    def ops(x):
        if isinstance(x, list):
            return sum(ops(y) for y in x)
        if not isinstance(x, dict):
            return 0
        t = x.get("physical_expr")
        if t == "column":
            cols.add(x["name"])
            return 1
        if t == "scalar_function_expr":
            name = (x.get("name") or "").lower()
            if name in ("char_length", "octet_length"):
                cols.add(name + "(" + x["args"][0]["name"] + ")")
                return 1
            return 1 + ops([a for a in x["args"] if "Utf8" not in json.dumps(a.get("value", ""))])
        if t == "in_list_expr":
            return len(x["list"]) * (ops(x["expr"]) + 3) + 1
        if t == "case_expr":
            return ops(x.get("else_expr")) + 1 + sum(ops(w) + ops(th) + 1 for w, th in x["when_then_expr"])
        return 1 + sum(ops(v) for k, v in x.items() if k != "physical_expr")
    return ops(e), len(cols)


def test_the_tree_generator_stays_within_the_program_limits():
    """At most one tree in four of a seed may be refused as too large on the GPU: the generator's depth is chosen so that -- by the reference's own
    count -- no seed has more than one such tree among its six programs' worth (96 operators, 8 columns per program)."""
    for seed in range(8):
        over = 0
        for exprs, pred in _trees(seed):
            big = [e for e in [pred] + [e for e, _ in exprs] if _program_size(e)[0] > 96 or _program_size(e)[1] > 8]
            over += bool(big)
        assert over * 4 <= 3, (seed, over)


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    ctx = GpuContext(0)
    yield ctx
    ctx.close()


def run(gpu, plan, sources, chunk=7_000, cols=COLS):
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        return collect(ctx, [[batches(t, chunk, cl)] for t, cl in sources])[0][0]
    finally:
        ctx.close()


_TABLES = {}


def shared_table(n, null_p=0.15):
    key = (n, null_p)
    if key not in _TABLES:
        _TABLES[key] = make_table(n, 100 + n, null_p)
    return _TABLES[key]


def every_function():
    out = [(name, fn(name, c("f"))) for name in MATH]
    out += [("trunc_" + u, trunc(u)) for u in ref.TRUNC_UNITS] + [("part_" + u, part(u)) for u in ref.PART_UNITS]
    out += [("octet_length", fn("octet_length", c("s"))), ("char_length", fn("char_length", c("s")))]
    return out


def _check_projection_and_filter(gpu, t):
    """Every function as a projected column (all of them in one plan), and each inside a filter of its own."""
    funcs = every_function()
    exprs = [(c("k"), "k")] + [(e, name) for name, e in funcs]
    rb = run(gpu, projection(exprs), [(t, COLS)])
    want = [t["k"]] + [ref.eval_rows(e, t, TYPES) for _, e in funcs]
    assert rb.schema.names == [n for _, n in exprs]
    got = pyrows(rb)
    assert len(got) == len(t["k"])
    assert got == want_rows(want)
    for (name, e), col in zip(funcs, want[1:]):
        ty = ref.result_type(e["name"])
        pivot = lit("Float64", 1.0) if ty == "Float64" else (lit("Int32", 3) if ty == "Int32" else c("t"))
        pred = binary(e, "GtEq" if ty != "Int32" else "Gt", pivot)
        rb = run(gpu, projection([(c("k"), "k")], filter_(pred)), [(t, COLS)])
        keep = ref.eval_rows(pred, t, TYPES, want="Boolean")
        assert rb.column(0).to_pylist() == [k for k, b in zip(t["k"], keep) if b is True], name


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_every_function_as_a_projection_and_inside_a_filter(gpu, n):
    _check_projection_and_filter(gpu, shared_table(n))


@pytest.mark.gpu
def test_every_function_over_all_null_arguments_and_an_empty_relation(gpu):
    t = dict(shared_table(8193))
    for col in ("f", "t", "s"):
        t[col] = [None] * 8193
    _check_projection_and_filter(gpu, t)
    _check_projection_and_filter(gpu, {name: [] for name in NAMES})


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(8))
def test_random_expression_trees(gpu, seed):
    from flock_amd import FlockGpuError, _ffi
    n = SIZES[seed % 3]
    t = shared_table(n, [0.15, 0.4][seed % 2])
    skipped = 0
    for exprs, pred in _trees(seed):
        try:
            rb = run(gpu, projection(exprs, filter_(pred)), [(t, COLS)])
        except FlockGpuError as e:
            assert e.code == _ffi.ERR_UNSUPPORTED and "expression too large" in str(e), str(e)
            skipped += 1
            continue
        keep = ref.eval_rows(pred, t, TYPES, want="Boolean")
        kept = {name: [v for v, b in zip(col, keep) if b is True] for name, col in t.items()}
        want = [ref.eval_rows(e, kept, TYPES) for e, _ in exprs]
        assert pyrows(rb) == want_rows(want), (seed, json.dumps(exprs), json.dumps(pred))
    assert skipped * 4 <= 3, skipped


@pytest.mark.gpu
def test_sqrt_is_bit_equal_to_the_correctly_rounded_root(gpu):
    vals = [5e-324, 1e-323, 2.2250738585072014e-308, 2.225073858507201e-308, 1e-310, 1e300, 1.7976931348623157e308, -1.0, -5e-324, -0.0, 0.0, -math.inf, math.inf, math.nan, 2.0, 3.0]
    for k in list(range(1, 200)) + [2**26 - 1, 2**26 + 1, 94906265, 94906267, 3037000499]:
        sq = float(k * k)
        vals += [sq, math.nextafter(sq, math.inf), math.nextafter(sq, 0.0)]
    r = np.random.default_rng(5)
    vals += [float(x) for x in np.abs(r.normal(0, 1e6, 4000))] + [float(x) for x in np.exp(r.uniform(-700, 700, 4000))]
    n = len(vals)
    t = {"k": list(range(n)), "i": [0] * n, "l": [0] * n, "f": vals, "t": [0] * n, "s": [""] * n}
    rb = run(gpu, projection([(fn("sqrt", c("f")), "r")]), [(t, COLS)])
    want = [math.nan if (v != v or v < 0) else math.sqrt(v) for v in vals]
    assert [ref.bits(v) for v in rb.column(0).to_pylist()] == [ref.bits(v) for v in want]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2049, 8193, 20_011])
def test_text_lengths_with_code_points_across_every_16_byte_position(gpu, n):
    """Values of 0, 1 and 70 bytes, 2-, 3- and 4-byte code points behind a prefix that grows by one byte from row to row (so that a code point straddles
    every 16-byte position of the byte stream), NULLs, and ONE value of 40 000 bytes -- longer than a round of the kernel's byte stream."""
    r = np.random.default_rng(n)
    vals = []
    for j in range(n):
        kind = j % 7
        prefix = "p" * (j % 17)
        vals.append(["", "a", prefix + "é", prefix + "€" + "q" * (j % 5), prefix + "\U0001F600", "w" * 70, prefix + "é€\U0001F600" * 3][kind])
    big = n // 2
    vals[big] = ("é€" * 8000)[: 40_000 // 5 * 2]          # 16 000 code points of 2 and 3 bytes = 40 000 bytes
    assert len(vals[big].encode()) == 40_000
    vals = [None if (r.random() < 0.15 and j != big) else v for j, v in enumerate(vals)]
    t = {"k": list(range(n)), "i": [0] * n, "l": [0] * n, "f": [0.0] * n, "t": [0] * n, "s": vals}
    cl, ol = fn("char_length", c("s")), fn("octet_length", c("s"))
    rb = run(gpu, projection([(c("k"), "k"), (cl, "c"), (ol, "o"), (binary(ol, "Minus", cl), "d")]), [(t, COLS)], chunk=6_000)
    want = [t["k"], ref.eval_rows(cl, t, TYPES), ref.eval_rows(ol, t, TYPES), ref.eval_rows(binary(ol, "Minus", cl), t, TYPES)]
    assert want[1][big] == 16_000 and want[2][big] == 40_000
    assert pyrows(rb) == want_rows(want)
    pred = binary(cl, "Gt", lit("Int32", 20))
    rb = run(gpu, projection([(c("k"), "k")], filter_(pred)), [(t, COLS)])
    keep = ref.eval_rows(pred, t, TYPES, want="Boolean")
    assert rb.column(0).to_pylist() == [k for k, b in zip(t["k"], keep) if b is True] and big in rb.column(0).to_pylist()


@pytest.mark.gpu
def test_strictness_of_function_arguments(gpu):
    """`floor(f) > 3` drops the rows whose f is NULL (the leaf may drop them at the scan); `date_part('hour', t) IS NULL OR i > 0` must KEEP the rows whose t is NULL."""
    t = shared_table(8193)
    for pred in (binary(fn("floor", c("f")), "Gt", lit("Float64", 3.0)),
                 binary(unary("is_null_expr", part("hour")), "Or", binary(c("i"), "Gt", lit("Int32", 0)))):
        rb = run(gpu, filter_(pred), [(t, COLS)])
        keep = ref.eval_rows(pred, t, TYPES, want="Boolean")
        want = [[v for v, b in zip(t[name], keep) if b is True] for name in NAMES]
        assert pyrows(rb) == want_rows(want)
    assert any(v is None for v in rb.column(NAMES.index("t")).to_pylist())


def _sort(inp, keys):
    return {"execution_plan": "sort_exec", "input": inp, "expr": [{"expr": e, "options": {"descending": False, "nulls_first": False}} for e in keys]}


@pytest.mark.gpu
def test_group_by_date_trunc_whole_and_staged_and_order_by_char_length(gpu):
    from flock_amd.stages import StagedRun, build_query_dag
    t = dict(shared_table(20_011))
    t["t"] = [None if v is None else 1436918400000 + (v % 3_000_000) for v in t["t"]]       # fifty minutes' worth of buckets
    rb = run(gpu, _group_by_minute(), [(t, COLS)])
    want = {}
    for ts, i in zip(t["t"], t["i"]):
        key = ref.call("date_trunc", ["minute", ts])
        cnt, mx = want.get(key, (0, None))
        want[key] = (cnt + 1, mx if i is None else i if mx is None else max(mx, i))
    got = sorted(pyrows(rb), key=repr)
    assert got == sorted([(k, v[0], v[1]) for k, v in want.items()], key=repr) and len(got) == 51          # fifty minutes and the NULL group
    assert pa.types.is_timestamp(rb.schema.field(0).type)
    staged = StagedRun(gpu, build_query_dag(_group_by_minute(parts=4)), instances=1, on_device=True)
    try:
        out = staged.run({"events": batches(t, 20_011)[0]})
    finally:
        staged.close()
    rows = []
    for b in out:
        rows += pyrows(b)
    assert sorted(rows, key=repr) == got
    # ORDER BY char_length(s), k -- NULL lengths last
    s = shared_table(8193)
    rb = run(gpu, projection([(c("k"), "k"), (c("s"), "s")], _sort(scan(), [fn("char_length", c("s")), c("k")])), [(s, COLS)])
    order = sorted(range(8193), key=lambda j: (s["s"][j] is None, ref.char_length(s["s"][j]) if s["s"][j] is not None else 0, j))
    assert rb.column(0).to_pylist() == order and rb.column(1).to_pylist() == [s["s"][j] for j in order]


@pytest.mark.gpu
def test_function_predicates_under_joins_and_a_repartition(gpu):
    left = shared_table(8193)
    rcols = [(n + "_r", ty) for n, ty in COLS]
    right = {n + "_r": v for n, v in shared_table(8193, 0.4).items()}
    pred = binary(binary(part("hour"), "GtEq", lit("Int32", 8)), "And", binary(fn("abs", c("f")), "Lt", lit("Float64", 60.0)))
    keep = ref.eval_rows(pred, left, TYPES, want="Boolean")
    kept = [k for k, b in zip(left["k"], keep) if b is True]
    assert 0 < len(kept) < 8193
    rkeys = {v for v in right["i_r"] if v is not None}

    def join(jt):
        l = {"execution_plan": "repartition_exec", "input": filter_(pred), "partitioning": {"Hash": [[c("i")], 4]}}
        r = {"execution_plan": "repartition_exec", "input": scan(rcols), "partitioning": {"Hash": [[c("i_r", rcols)], 4]}}
        out = COLS + (rcols if jt == "Inner" else [])
        return {"execution_plan": "hash_join_exec", "left": l, "right": r, "join_type": jt, "mode": "Partitioned", "on": [[c("i"), c("i_r", rcols)]],
                "schema": {"fields": [_field(n, ty) for n, ty in out], "metadata": {}}}
    semi = run(gpu, join("Semi"), [(left, COLS), (right, rcols)])
    assert semi.column(0).to_pylist() == [k for k in kept if left["i"][k] in rkeys]
    inner = run(gpu, projection([(c("k"), "k"), (c("k_r", COLS + rcols), "k_r")], join("Inner"), {**TYPES, "k_r": "Int32"}), [(left, COLS), (right, rcols)])
    by_key = {}
    for k, v in zip(right["k_r"], right["i_r"]):
        by_key.setdefault(v, []).append(k)
    want = sorted((k, kr) for k in kept if left["i"][k] is not None for kr in by_key.get(left["i"][k], []))
    assert sorted(zip(inner.column(0).to_pylist(), inner.column(1).to_pylist())) == want and want
    # Filter -> Repartition at the root
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([{"execution_plan": "repartition_exec", "input": filter_(pred), "partitioning": {"Hash": [[c("k")], 4]}}], gpu=gpu)
    try:
        parts = collect(ctx, [[batches(left, 7_000)]])           # one list of batches per partition
    finally:
        ctx.close()
    assert len(parts) == 4 and sorted(k for part in parts for b in part for k in b.column(0).to_pylist()) == kept


BID = [("auction", "Int32"), ("bidder", "Int32"), ("price", "Int32"), ("b_date_time", "ts")]


@pytest.mark.gpu
def test_now_and_q12(gpu):
    from flock_amd.runtime import ExecutionContext
    r = np.random.default_rng(12)
    n = 20_011
    bid = {"auction": [int(x) for x in r.integers(1000, 2000, n)], "bidder": [int(x) for x in r.integers(0, 300, n)], "price": [int(x) for x in r.integers(1, 10**6, n)],
           "b_date_time": [1436918400000 + 13 * j for j in range(n)]}
    p_time = ExecutionContext([open(os.path.join(PLANS, "q12_p_time.json")).read()], gpu=gpu)
    q12 = ExecutionContext([open(os.path.join(PLANS, "q12.json")).read()], gpu=gpu)
    try:
        p_time.feed_data_sources([[batches(bid, 7_000, BID)]])
        before = time.time_ns() // 1_000_000
        first = p_time.execute()[0][0]
        after = time.time_ns() // 1_000_000
        assert first.schema.names == [cn for cn, _ in BID] + ["p_time"] and pa.types.is_timestamp(first.schema.field(4).type)
        assert [first.column(j).to_pylist() for j in range(3)] == [bid["auction"], bid["bidder"], bid["price"]]
        stamps = set(first.column(4).cast(pa.int64()).to_pylist())
        assert len(stamps) == 1
        now1 = stamps.pop()
        assert before - 1 <= now1 <= after + 1, (before, now1, after)
        time.sleep(0.005)
        second = p_time.execute()[0][0]
        now2 = set(second.column(4).cast(pa.int64()).to_pylist())
        assert len(now2) == 1 and now2.pop() >= now1
        # the result, left on the device, feeds q12's GROUP BY bidder
        p_time.execute_retain()
        q12.feed_from([p_time])
        out = q12.execute()[0][0]
        after = time.time_ns() // 1_000_000
        rows = pyrows(out)
        counts = np.bincount(np.array(bid["bidder"]), minlength=300)
        assert sorted(r[0] for r in rows) == [b for b in range(300) if counts[b]]
        stamp = {r[2] for r in rows}
        assert len(stamp) == 1 and now1 <= next(iter(stamp)) <= after + 1
        for b, cnt, lo, hi in rows:
            assert cnt == counts[b] and lo == hi
    finally:
        q12.close()
        p_time.close()
