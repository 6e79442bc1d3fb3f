"""CAST(x AS Int32 / Int64 / UInt64 / Timestamp(ms)) / TRY_CAST of Utf8 values (flock_amd/csrc/textnum.hpp A-TN1..A-TN6): as projected columns, in
predicates, under arithmetic and CASE, as GROUP BY / ORDER BY / DISTINCT keys, aggregate arguments and join keys, over columns, slices, text CASEs and
numbers cast to Utf8, in stage plans whole and split.  Every GPU comparison is exact -- values and validity -- against tests/parse_text_ref.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import parse_text_ref as ref
from cast_text_ref import cast_utf8, int_text, ts_text
from parse_text_ref import TS, TS_MAX, TS_MIN, cast_to
from text_expr_ref import case, lit_utf8
from text_slice_ref import lit, sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")

R = 1024             # textnum.hip kParseRows: rows of a workgroup of the parse kernel
ROUND = 16384        # textnum.hip kParseRoundBytes: bytes of a staging round

COLS = [("k", "Int32"), ("s", "Utf8"), ("d", "Utf8"), ("i", "Int32")]
TYPES = dict(COLS)
PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Timestamp": pa.timestamp("ms"), "Utf8": pa.string()}


def _dt(t):
    return TS if t == "Timestamp" else t


def _field(name, t, nullable=True):
    return {"data_type": _dt(t), "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


def _fields(cols):
    return {"fields": [_field(n, t) for n, t in cols], "metadata": {}}


def c(name, cols=COLS):
    return {"physical_expr": "column", "name": name, "index": [n for n, _ in cols].index(name)}


def binary(l, op, r):
    return {"physical_expr": "binary_expr", "left": l, "op": op, "right": r}


def scan(cols=COLS):
    return {"execution_plan": "memory_exec", "schema": _fields(cols), "projection": list(range(len(cols)))}


def projection(exprs, inp=None):
    """exprs: (expression, name, type)."""
    return {"execution_plan": "projection_exec", "expr": [[e, n] for e, n, _ in exprs], "input": scan() if inp is None else inp, "schema": _fields([(n, t) for _, n, t in exprs])}


def filter_(pred, inp=None):
    return {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096, "input": {"execution_plan": "filter_exec", "predicate": pred, "input": scan() if inp is None else inp}}


def sort_(inp, keys):
    return {"execution_plan": "sort_exec", "input": inp, "expr": [{"expr": e, "options": {"descending": d, "nulls_first": False}} for e, d in keys]}


def group_by(key_expr, key_type, aggs, parts=None, cols=COLS, key="g"):
    """SELECT <key>, <aggs> GROUP BY 1 -- Partial / [Hash] / Final.  aggs: (function, name, type, argument)."""
    entries = [{"aggregate_expr": f, "name": n, "data_type": t, "nullable": True, "expr": a} for f, n, t, a in aggs]
    kc = {"physical_expr": "column", "name": key, "index": 0}
    partial = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [[key_expr, key]], "aggr_expr": entries, "input": scan(cols), "input_schema": _fields(cols),
               "schema": _fields([(key, key_type)] + [("%s[%s]" % (n, f), t) for f, n, t, _ in aggs])}
    mid = partial
    if parts:
        mid = {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096, "input": {"execution_plan": "repartition_exec", "input": partial, "partitioning": {"Hash": [[kc], parts]}}}
    return {"execution_plan": "hash_aggregate_exec", "mode": "FinalPartitioned" if parts else "Final", "group_expr": [[kc, key]], "aggr_expr": entries, "input": mid,
            "input_schema": _fields(cols), "schema": _fields([(key, key_type)] + [(n, t) for _, n, t, _ in aggs])}


def ungrouped(aggs, cols=COLS):
    entries = [{"aggregate_expr": f, "name": n, "data_type": t, "nullable": True, "expr": a} for f, n, t, a in aggs]
    partial = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [], "aggr_expr": entries, "input": scan(cols), "input_schema": _fields(cols),
               "schema": _fields([("%s[%s]" % (n, f), t) for f, n, t, _ in aggs])}
    return {"execution_plan": "hash_aggregate_exec", "mode": "Final", "group_expr": [], "aggr_expr": entries, "input": {"execution_plan": "coalesce_partitions_exec", "input": partial},
            "input_schema": _fields(cols), "schema": _fields([(n, t) for _, n, t, _ in aggs])}


def distinct(key_expr, key_type, key="x"):
    kc = {"physical_expr": "column", "name": key, "index": 0}
    part = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [[key_expr, key]], "aggr_expr": [], "input": scan(), "input_schema": _fields(COLS), "schema": _fields([(key, key_type)])}
    rep = {"execution_plan": "repartition_exec", "input": part, "partitioning": {"Hash": [[kc], 4]}}
    return {"execution_plan": "hash_aggregate_exec", "mode": "FinalPartitioned", "group_expr": [[kc, key]], "aggr_expr": [], "input": rep, "input_schema": _fields(COLS), "schema": _fields([(key, key_type)])}


COUNT = ("count", "COUNT(UInt8(1))", "UInt64", lit("UInt8", 1))


def batch(t, a, b, cols=COLS):
    return pa.record_batch([pa.array(t[cn][a:b], PA[ty]) for cn, ty in cols], names=[cn for cn, _ in cols])


def batches(t, parts, cols=COLS):
    n = len(t[cols[0][0]])
    step = max((n + parts - 1) // parts, 1)
    return [batch(t, a, min(a + step, n), cols) for a in range(0, max(n, 1), step)]


def refused(plan, *words):
    from flock_amd import _ffi
    from flock_amd.runtime import FlockGpuError, explain
    with pytest.raises(FlockGpuError) as e:
        explain(plan)
    assert e.value.code == _ffi.ERR_UNSUPPORTED, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


# ------------------------------------------------------------------ the values
INT_POOL = ["0", "7", "-1", "42", "+13", "007", "2147483647", "-2147483648", "2147483648", "9223372036854775807", "-9223372036854775808", "9223372036854775808", "18446744073709551615",
            "18446744073709551616", "", "-", "x", "12a", " 1", "1 ", "00000000000000000000000000123", "-000000000000000000000000000000000000009", "99999", "123456789012", "-98765432101234"]
TS_POOL = ["2015-07-15", "2015-07-15 09", "2015-07-15T09:08", "2015-07-15 09:08:07", "2015-07-15 09:08:07.1", "2015-07-15T09:08:07.12", "2015-07-15 09:08:07.123", "1969-12-31 23:59:59.999",
           "0000-01-01 00:00:00", "9999-12-31 23:59:59.999", "1900-02-29", "1600-02-29", "2015-07-15 24:00", "", "2015-07-15 09:08:07.1234", "2015-07-1", "x", "2016-02-29 23:59:59"]


def make_table(n):
    """Valid and invalid numbers and timestamps of every length; NULLs at every workgroup's first and last row and every 97th."""
    t = {"k": list(range(n)), "s": [INT_POOL[(j * 7) % len(INT_POOL)] for j in range(n)], "d": [TS_POOL[(j * 5) % len(TS_POOL)] for j in range(n)], "i": [j % 10 for j in range(n)]}
    for j in range(n):
        if j % R in (0, R - 1) or j % 97 == 5:
            t["s"][j] = None
            if j % 2:
                t["d"][j] = None
    return t


_TABLES = {}


def shared_table(n):
    if n not in _TABLES:
        _TABLES[n] = make_table(n)
    return _TABLES[n]


INT_TARGETS = ("Int32", "Int64", "UInt64")
EVERY = [(cast_to(c("s"), ty, try_cast=True), ty) for ty in INT_TARGETS] + [(cast_to(c("d"), "Timestamp", try_cast=True), "Timestamp")]


# ------------------------------------------------------------------ CPU: the reference
def test_reference_by_hand():
    for (s, ty), v in ref.BY_HAND.items():
        assert ref.parse_one(s, ty) == v, (s, ty)
    assert ref.parse(["5", None, "x", "-0"], "Int64", try_cast=True) == [5, None, None, 0]
    with pytest.raises(ref.ParseError):
        ref.parse(["5", "x"], "Int64")
    assert ref.parse(["5", None], "Int64") == [5, None]
    assert ref.parse_ts("2015-07-15 09:08:07.123") == 1436951287123 and ref.parse_ts("2015-07-15 09:08:07.12") == 1436951287120
    assert ref.parse_ts("1970-01-01") == 0 and ref.parse_ts("1970-01-01T00:00:00.001") == 1 and ref.parse_ts("1970-01-01t00") is None


def test_reference_against_pyarrow():
    """The seeded corpus, value by value, as 'pyarrow raises'; the three classes where the rules differ are left out, and are under 5 % of it."""
    cp = ref.corpus()
    assert len(cp) >= 3000 and set(ref.EDGES) <= set(cp)
    left_out = checked = parsed = 0
    for ty in ref.TARGETS:
        for s in cp:
            if ref.differs_from_pyarrow(s, ty):
                left_out += 1
                continue
            try:
                got = pc.cast(pa.array([s], pa.string()), PA[ty])
                got = got.cast(pa.int64())[0].as_py() if ty == "Timestamp" else got[0].as_py()
            except pa.ArrowInvalid:
                got = None
            assert got == ref.parse_one(s, ty), (s, ty, got, ref.parse_one(s, ty))
            checked += 1
            parsed += got is not None
    assert left_out < 0.05 * (left_out + checked), (left_out, checked)
    assert parsed > 0.1 * checked and parsed < 0.9 * checked, (parsed, checked)     # values that parse and values that do not, both in numbers
    # the three classes, pinned by hand
    for s, ty in (("+5", "Int64"), ("0x10", "Int64"), ("0000-01-01 00:00:00", "Timestamp")):
        assert ref.differs_from_pyarrow(s, ty) and (s, ty) in ref.BY_HAND


def test_textnum_on_the_host():
    """textnum.hpp as a stand-alone host program: against strtoull and the rules on the edge table, and the round trip through numtext.hpp."""
    exe = os.path.join(ROOT, "tests", "cpp", "textnum_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "flock_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "textnum_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "textnum_test: ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ CPU: parsing, explain, refusals
def test_a_projected_cast_explains_with_its_type():
    from flock_amd.runtime import explain
    for ty, shown in (("Int32", "Int32"), ("Int64", "Int64"), ("UInt64", "UInt64"), ("Timestamp", "Timestamp(ms)")):
        first = explain(projection([(cast_to(c("s"), ty), "x", ty), (c("k"), "k", "Int32")])).splitlines()[0]
        assert first.startswith("Project(x = CAST(s AS %s)) [x:%s, k:Int32]" % (shown, shown)), first
        first = explain(projection([(cast_to(c("s"), ty, try_cast=True), "x", ty)])).splitlines()[0]
        assert first.startswith("Project(x = TRY_CAST(s AS %s)) [x:%s]" % (shown, shown)), first
    first = explain(projection([(cast_to(sl("left", c("s"), lit("Int64", 4)), "Int32"), "x", "Int32")])).splitlines()[0]
    assert first.startswith("Project(x = CAST(left(s, 4) AS Int32)) [x:Int32]"), first
    first = explain(projection([(binary(cast_to(sl("split_part", c("s"), lit("Utf8", "="), lit("Int64", 2)), "Int64"), "Plus", lit("Int64", 1)), "x", "Int64")])).splitlines()[0]
    assert first.startswith("Project(x = CAST(split_part(s, '=', 2) AS Int64) + 1) [x:Int64]"), first
    first = explain(projection([(cast_to(sl("left", cast_utf8(cast_to(c("d"), "Timestamp")), lit("Int64", 10)), "Timestamp"), "day", "Timestamp")])).splitlines()[0]
    assert first.startswith("Project(day = CAST(left(CAST(CAST(d AS Timestamp(ms)) AS Utf8), 10) AS Timestamp(ms))) [day:Timestamp(ms)]"), first
    txt = explain(projection([(c("k"), "k", "Int32")], filter_(binary(cast_to(c("s"), "Int64"), "Gt", lit("Int64", 100)))))
    assert "Filter(CAST(s AS Int64) > 100)" in txt, txt
    txt = explain(group_by(cast_to(c("s"), "Int64"), "Int64", [COUNT], parts=4))
    assert "Project(#4 = CAST(s AS Int64))" in txt and "#4:Int64" in txt, txt
    txt = explain(sort_(scan(), [(cast_to(c("d"), "Timestamp", try_cast=True), True)]))
    assert "Project(#4 = TRY_CAST(d AS Timestamp(ms)))" in txt and "#4:Timestamp(ms)" in txt, txt


def test_the_fixture_explains_and_is_no_fused_query():
    from flock_amd import _ffi, build
    from flock_amd.runtime import explain
    raw = open(os.path.join(PLANS, "person_card_prefix.json")).read()
    txt = explain(raw)
    assert "Project(#1 = CAST(left(credit_card, 4) AS Int32)) [credit_card:Utf8, #1:Int32]" in txt and txt.splitlines()[0].startswith("Project [prefix:Int32, COUNT(UInt8(1)):UInt64]"), txt
    assert "fused" not in txt
    build.build()
    lib = _ffi.load()
    got = C.c_int(-1)
    assert lib.flockgpu_plan_recognise(raw.encode(), len(raw.encode()), C.byref(got)) == _ffi.OK and got.value == 0


def test_refusals_by_name():
    p = lambda e, ty="Int64": projection([(e, "x", ty)])
    for tag, tc in (("cast_expr: ", False), ("try_cast_expr: ", True)):
        refused(p(cast_to(c("s"), "Float64", try_cast=tc), "Float64"), tag + "CAST of a Utf8 value to Float64")
        refused(p(cast_to(sl("left", c("s"), lit("Int64", 2)), "Float64", try_cast=tc), "Float64"), tag + "CAST of a Utf8 value to Float64")
        refused(p(cast_to(c("s"), "Boolean", try_cast=tc)), tag + "CAST of a Utf8 value to Boolean")
        for unit in ("Second", "Microsecond", "Nanosecond"):
            e = {"physical_expr": "try_cast_expr" if tc else "cast_expr", "expr": c("s"), "cast_type": {"Timestamp": [unit, None]}}
            refused(p(e), tag + "CAST of a Utf8 value to a Timestamp of another unit than Millisecond")
        refused(p(cast_to(lit_utf8("5"), "Int64", try_cast=tc)), tag + "CAST of a Utf8 literal", "a literal operand")
        refused(p(cast_to(cast_utf8(lit_utf8("5")), "Int32", try_cast=tc)), tag + "CAST of a Utf8 literal")
    # in a predicate and as a key alike
    refused(filter_(binary(cast_to(c("s"), "Float64"), "Gt", lit("Float64", 1.0))), "cast_expr: CAST of a Utf8 value to Float64")
    refused(group_by(cast_to(lit_utf8("5"), "Int64"), "Int64", [COUNT]), "cast_expr: CAST of a Utf8 literal")
    # what was refused before keeps its words
    refused(p(cast_to(c("k"), "Boolean")), "cast to an unsupported type")
    refused(projection([(case([(binary(c("k"), "Gt", lit("Int32", 0)), cast_to(c("s"), "Int32"))], lit_utf8("x")), "y", "Utf8")]), "CASE branches of different types")
    refused(p(cast_to(sl("left", lit_utf8("abc"), lit("Int64", 2)), "Int64")), "the value argument is a literal")


def test_a_group_by_on_the_cast_splits_into_two_stages_that_both_explain():
    from flock_amd.runtime import explain
    from flock_amd.stages import build_query_dag, split_at_repartitions
    plan = group_by(cast_to(c("s"), "Int64"), "Int64", [COUNT], parts=4)
    for dag in (build_query_dag(plan), split_at_repartitions(plan)):
        assert len(dag) == 2
        texts = [explain(s.plan) for s in dag]
        assert "CAST(s AS Int64)" in texts[0] and "Aggregate(Partial)" in texts[0] and "Aggregate(FinalPartitioned)" in texts[1] and "g:Int64" in texts[1], texts
    raw = json.loads(open(os.path.join(PLANS, "person_card_prefix.json")).read())
    dag = build_query_dag(raw)
    assert len(dag) == 2 and "CAST(left(credit_card, 4) AS Int32)" in explain(dag[0].plan) and "prefix:Int32" in explain(dag[1].plan)


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    ctx = GpuContext(0)
    yield ctx
    ctx.close()


def run(gpu, plan, sources):
    """sources: one (table, columns, batches) per leaf."""
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        return collect(ctx, [[batches(t, parts, cl)] for t, cl, parts in sources])[0][0]
    finally:
        ctx.close()


def values_of(col):
    """A result column as Python values, None for NULL; a timestamp as its millisecond count."""
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    return (col.cast(pa.int64()) if pa.types.is_timestamp(col.type) else col).to_pylist()


def check(gpu, exprs, t, parts=1, cols=COLS, want=None):
    """Projects k and every (expression, type); each column equals the reference in value and validity, and has the cast's type."""
    plan = projection([(c("k", cols), "k", "Int32")] + [(e, "x%d" % j, ty) for j, (e, ty) in enumerate(exprs)], inp=scan(cols))
    rb = run(gpu, plan, [(t, cols, parts)])
    assert rb.num_rows == len(t["k"]) and rb.column(0).to_pylist() == t["k"]
    for j, (e, ty) in enumerate(exprs):
        got = rb.column(1 + j)
        assert got.type == PA[ty], (j, got.type)
        g = values_of(got)
        assert g == want[j], (j, json.dumps(e)[:160], [(a, b) for a, b in zip(g, want[j]) if a != b][:5])
    return rb


_WANT = {}


def wanted(n):
    """The reference's columns for EVERY over shared_table(n): computed once."""
    if n not in _WANT:
        t = shared_table(n)
        _WANT[n] = [ref.parse(t["s"], ty, try_cast=True) for ty in INT_TARGETS] + [ref.parse(t["d"], "Timestamp", try_cast=True)]
    return _WANT[n]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, R - 1, R, R + 1, 2 * R + 3])
def test_row_counts_around_the_wave_and_the_workgroup_in_one_batch_and_in_three(gpu, n):
    t = shared_table(n)
    a = check(gpu, EVERY, t, parts=1, want=wanted(n))
    b = check(gpu, EVERY, t, parts=3, want=wanted(n))
    for j in range(1, a.num_columns):
        assert values_of(a.column(j)) == values_of(b.column(j)), j
    if n >= R:
        w = wanted(n)
        assert w[1][R - 1] is None and w[1][1] is not None and any(v is None for v in w[3]) and sum(v is not None for v in w[3]) > n // 2 and sum(v is not None for v in w[0]) > n // 4


@pytest.mark.gpu
def test_ten_thousand_values_whose_bytes_cross_the_staging_round_in_every_workgroup(gpu):
    """Numbers of 18 to 20 digits, every 32nd behind 700 zeros (the plain path): a workgroup's 1024 rows span more than two rounds, rows straddle the seams."""
    n = 10_000
    r = np.random.default_rng(5)
    vals = [int(x) for x in r.integers(10**17, 2**63 - 1, n)]
    t = {"k": list(range(n)), "s": [("0" * 700 if j % 32 == 7 else "") + str(v * (2 if j % 3 == 0 else 1)) for j, v in enumerate(vals)],
         "d": ts_text([int(x) for x in r.integers(TS_MIN, TS_MAX, n)]), "i": [0] * n}
    for j in (0, 5, R - 1, R, 4 * R + 1):
        t["s"][j] = None
    span = sum(len(s) for s in t["s"][R:2 * R] if s is not None)
    assert span > 2 * ROUND and sum(len(s) for s in t["d"][R:2 * R]) > ROUND
    want = [ref.parse(t["s"], "Int64", try_cast=True), ref.parse(t["s"], "UInt64", try_cast=True), ref.parse(t["d"], "Timestamp")]
    assert sum(v is None and s is not None for v, s in zip(want[0], t["s"])) > 100 and all(v is not None for j, v in enumerate(want[1]) if t["s"][j] is not None)
    for parts in (1, 3):
        check(gpu, [(cast_to(c("s"), "Int64", try_cast=True), "Int64"), (cast_to(c("s"), "UInt64", try_cast=True), "UInt64"), (cast_to(c("d"), "Timestamp"), "Timestamp")], t, parts=parts, want=want)


@pytest.mark.gpu
def test_values_at_every_misalignment_a_value_longer_than_a_round_empties_and_all_null(gpu):
    # lengths 1..17 in turn: the values begin at every offset modulo 16
    n = 600
    t = {"k": list(range(n)), "s": [str(10 ** (j % 17) + j % 7)[: j % 17 + 1] for j in range(n)], "d": ["2015-07-15 09:08:07.12"[: [10, 13, 16, 19, 21, 22][j % 6]] for j in range(n)], "i": [0] * n}
    starts = np.cumsum([0] + [len(s) for s in t["s"]])[:-1]
    assert {int(x) % 16 for x in starts} == set(range(16)) and {int(x) % 16 for x in np.cumsum([0] + [len(s) for s in t["d"]])[:-1]} == set(range(16))
    check(gpu, [(cast_to(c("s"), "Int64"), "Int64"), (cast_to(c("s"), "UInt64"), "UInt64"), (cast_to(c("d"), "Timestamp"), "Timestamp")], t,
          want=[ref.parse(t["s"], "Int64"), ref.parse(t["s"], "UInt64"), ref.parse(t["d"], "Timestamp")])
    # one value longer than a round, between short ones
    t = {"k": list(range(9)), "s": ["1", "-2", "0" * 40_000 + "7", "3", "", None, "-" + "0" * 40_000 + "8", "0" * 40_000 + "x", "5"], "d": [None] * 9, "i": [0] * 9}
    assert len(t["s"][2]) > 2 * ROUND
    for ty in INT_TARGETS:
        want = ref.parse(t["s"], ty, try_cast=True)
        assert want[2] == 7 and want[4] is None and want[7] is None and want[6] == (None if ty == "UInt64" else -8)
        rb = check(gpu, [(cast_to(c("s"), ty, try_cast=True), ty), (cast_to(c("d"), "Timestamp"), "Timestamp")], t, want=[want, [None] * 9])     # (d: an all-NULL column)
        assert rb.column(2).null_count == 9


def _fails(gpu, exprs, t, *words):
    from flock_amd import _ffi
    from flock_amd.runtime import FlockGpuError
    with pytest.raises(FlockGpuError) as e:
        check(gpu, exprs, t, want=None)
    assert e.value.code == _ffi.ERR_INVALID, str(e.value)
    for w in ("cast_expr", "Utf8") + words:
        assert w in str(e.value), (w, str(e.value))


@pytest.mark.gpu
def test_the_edge_table_under_try_cast_and_one_bad_row_under_cast(gpu):
    edges = ref.EDGES + [None]
    n = len(edges)
    t = {"k": list(range(n)), "s": edges, "d": edges, "i": [0] * n}
    exprs = [(cast_to(c("s"), ty, try_cast=True), ty) for ty in ref.TARGETS]
    want = [ref.parse(edges, ty, try_cast=True) for ty in ref.TARGETS]
    for (s, ty), v in ref.BY_HAND.items():
        assert want[ref.TARGETS.index(ty)][edges.index(s)] == v
    check(gpu, exprs, t, want=want)
    # cast_expr: one bad row fails the call by name; the same table without it succeeds
    for ty, shown, good, bad in (("Int32", "Int32", ["1", None, "-2147483648", "+7"], "2147483648"), ("Int64", "Int64", ["1", None, "007"], "1e3"), ("UInt64", "UInt64", ["1", None, "0"], "-0"),
                                 ("Timestamp", "Timestamp(ms)", ["2015-07-15", None, "1600-02-29", "2015-07-15T23:59:59.9"], "2015-07-15 23:59:60"), ("Int64", "Int64", ["5"], "")):
        rows = good * 300
        ok = {"k": list(range(len(rows))), "s": rows, "d": rows, "i": [0] * len(rows)}
        check(gpu, [(cast_to(c("s"), ty), ty)], ok, want=[ref.parse(rows, ty)])
        rows = list(rows)
        rows[len(rows) // 2 + 1] = bad
        broken = dict(ok, s=rows)
        _fails(gpu, [(cast_to(c("s"), ty), ty)], broken, shown)
        # ... even under a CASE that would not pick the row (every branch is evaluated for every row)
        _fails(gpu, [(case_num([(binary(c("k"), "Lt", lit("Int32", 0)), cast_to(c("s"), ty))], None), ty)], broken, shown)
        check(gpu, [(cast_to(c("s"), ty, try_cast=True), ty)], broken, want=[ref.parse(rows, ty, try_cast=True)])


def case_num(whens, els=None):
    return {"physical_expr": "case_expr", "expr": None, "when_then_expr": [[w, th] for w, th in whens], "else_expr": els}


@pytest.mark.gpu
def test_the_round_trip_through_utf8_is_the_identity(gpu):
    n = 3 * R + 11
    r = np.random.default_rng(23)
    cols = [("k", "Int32"), ("a", "Int32"), ("b", "Int64"), ("u", "UInt64"), ("t", "Timestamp")]
    t = {"k": list(range(n)), "a": [int(x) for x in r.integers(-2**31, 2**31, n)], "b": [int(x) >> int(s) for x, s in zip(r.integers(-2**63, 2**63 - 1, n), r.integers(0, 63, n))],
         "u": [int(x) >> int(s) for x, s in zip(r.integers(0, 2**64 - 1, n, dtype=np.uint64), r.integers(0, 64, n))], "t": [int(x) for x in r.integers(TS_MIN, TS_MAX, n)]}
    for name, extremes in (("a", [-2**31, 2**31 - 1, 0, -1]), ("b", [-2**63, 2**63 - 1, 0, -1]), ("u", [0, 2**64 - 1, 2**63, 10**19]), ("t", [TS_MIN, TS_MAX, 0, -1, 999, 1000])):
        for j, v in enumerate(extremes):
            t[name][7 + 3 * j] = v
        for j in range(0, n, 53):
            t[name][j] = None
    exprs = [(cast_to(cast_utf8(c(name, cols)), ty), ty) for name, ty in cols[1:]]
    assert int_text(t["b"])[7] == "-9223372036854775808" and ts_text(t["t"])[7] == "0000-01-01 00:00:00"
    for parts in (1, 3):
        check(gpu, exprs, t, parts=parts, cols=cols, want=[t[name] for name, _ in cols[1:]])


@pytest.mark.gpu
def test_operands_a_column_slices_and_a_text_case_under_arithmetic_case_in_and_is_null(gpu):
    n = R + 77
    cards = ["%04d %04d %04d %04d" % ((j * 37) % 10_000, j % 7, 3, 4) for j in range(n)]
    urls = ["https://x.io/%d/item" % (j * 11 - 40) if j % 5 else "https://x.io//item" if j % 10 else "no-slash" for j in range(n)]      # field 4 of '/': a number, '' or nothing
    t = {"k": list(range(n)), "s": cards, "d": urls, "i": [j % 10 for j in range(n)]}
    for j in (0, 9, R - 1, R):
        t["s"][j] = t["d"][j] = None
    prefix = cast_to(sl("left", c("s"), lit("Int64", 4)), "Int32")
    field = cast_to(sl("split_part", c("d"), lit("Utf8", "/"), lit("Int64", 4)), "Int64", try_cast=True)
    second = cast_to(sl("split_part", sl("left", c("s"), lit("Int64", 9)), lit("Utf8", " "), lit("Int64", 2)), "UInt64")
    label = case([(binary(c("i"), "Lt", lit("Int32", 3)), sl("left", c("s"), lit("Int64", 4))), (binary(c("i"), "Lt", lit("Int32", 6)), lit_utf8("77")), (binary(c("i"), "Lt", lit("Int32", 8)), cast_utf8(c("k")))],
                 lit_utf8("none"))
    w_prefix = [None if s is None else int(s[:4]) for s in cards]
    w_field = [None if u is None or u.count("/") < 3 else ref.parse_one(u.split("/")[3], "Int64") for u in urls]
    w_second = [None if s is None else int(s[5:9]) for s in cards]
    texts = [None if (cards[j] is None and t["i"][j] < 3) else cards[j][:4] if t["i"][j] < 3 else "77" if t["i"][j] < 6 else str(j) if t["i"][j] < 8 else "none" for j in range(n)]
    w_label = ref.parse(texts, "Int64", try_cast=True)
    assert any(v is None for v in w_field[1:20]) and any(v is not None and v < 0 for v in w_field) and w_label[8:10] == [None, None] and w_label[3] == 77 and w_label[6] == 6
    plus = binary(cast_to(prefix, "Int64"), "Plus", field)
    picked = case_num([(binary(prefix, "Gt", lit("Int32", 5000)), field), ({"physical_expr": "is_null_expr", "arg": field}, lit("Int64", -1))], cast_to(prefix, "Int64"))
    w_plus = [None if a is None or b is None else a + b for a, b in zip(w_prefix, w_field)]
    w_picked = [(b if a is not None and a > 5000 else -1 if b is None else a) for a, b in zip(w_prefix, w_field)]
    exprs = [(prefix, "Int32"), (field, "Int64"), (second, "UInt64"), (cast_to(label, "Int64", try_cast=True), "Int64"), (plus, "Int64"), (picked, "Int64"), (prefix, "Int32")]
    check(gpu, exprs, t, parts=2, want=[w_prefix, w_field, w_second, w_label, w_plus, w_picked, w_prefix])
    # IN and IS NULL as predicates
    inl = {"physical_expr": "in_list_expr", "expr": prefix, "list": [lit("Int32", 37), lit("Int32", 74), lit("Int32", 9990)], "negated": False}
    rb = run(gpu, projection([(c("k"), "k", "Int32")], filter_(inl)), [(t, COLS, 1)])
    assert rb.column(0).to_pylist() == [j for j in range(n) if w_prefix[j] in (37, 74, 9990)] and rb.num_rows >= 2
    rb = run(gpu, projection([(c("k"), "k", "Int32")], filter_({"physical_expr": "is_null_expr", "arg": field})), [(t, COLS, 1)])
    assert rb.column(0).to_pylist() == [j for j in range(n) if w_field[j] is None]


def _rows(b):
    return list(zip(*[values_of(b.column(j)) for j in range(b.num_columns)]))


@pytest.mark.gpu
def test_the_cast_in_a_filter_as_an_aggregate_argument_and_as_a_key(gpu):
    n = 2 * R + 9
    t = {"k": list(range(n)), "s": [str((j * 7919) % 1000 - 300) if j % 11 else None for j in range(n)], "d": [None] * n, "i": [j % 10 for j in range(n)]}
    v = ref.parse(t["s"], "Int64")
    e = cast_to(c("s"), "Int64")
    rb = run(gpu, projection([(c("k"), "k", "Int32"), (c("s"), "s", "Utf8")], filter_(binary(e, "Gt", lit("Int64", 100)))), [(t, COLS, 2)])
    keep = [j for j in range(n) if v[j] is not None and v[j] > 100]
    assert rb.column(0).to_pylist() == keep and rb.column(1).to_pylist() == [t["s"][j] for j in keep] and 0 < len(keep) < n
    # SUM(CAST(s AS Int64)), ungrouped and grouped by i
    sm = ("sum", "SUM(x)", "Int64", e)
    assert _rows(run(gpu, ungrouped([sm, COUNT]), [(t, COLS, 1)])) == [(sum(x for x in v if x is not None), n)]
    want = {}
    for g, x in zip(t["i"], v):
        a, b = want.get(g, (None, 0))
        want[g] = (a if x is None else x if a is None else a + x, b + 1)
    for parts in (None, 4):
        assert sorted(_rows(run(gpu, group_by(c("i"), "Int32", [sm, COUNT], parts=parts), [(t, COLS, 2)]))) == sorted((g, a, b) for g, (a, b) in want.items())
    # GROUP BY / DISTINCT / ORDER BY on the cast
    mod = cast_to(sl("right", c("s"), lit("Int64", 1)), "Int32")          # the last digit
    keys = [None if s is None else int(s[-1]) for s in t["s"]]
    cnt = {}
    for g in keys:
        cnt[g] = cnt.get(g, 0) + 1
    for parts in (None, 4):
        assert sorted(_rows(run(gpu, group_by(mod, "Int32", [COUNT], parts=parts), [(t, COLS, 1)])), key=repr) == sorted(cnt.items(), key=repr) and len(cnt) == 11
    assert sorted(values_of(run(gpu, distinct(mod, "Int32"), [(t, COLS, 1)]).column(0)), key=repr) == sorted(set(keys), key=repr)
    for desc in (False, True):
        rb = run(gpu, projection([(c("k"), "k", "Int32")], sort_(scan(), [(e, desc), (c("k"), False)])), [(t, COLS, 1)])
        some = sorted((j for j in range(n) if v[j] is not None), key=lambda j: (-v[j] if desc else v[j], j))
        assert rb.column(0).to_pylist() == some + [j for j in range(n) if v[j] is None], desc


@pytest.mark.gpu
def test_a_text_id_joins_an_int64_id_inner_and_semi(gpu):
    n = 500
    lcols = [("k", "Int32"), ("id", "Int64")]
    left_t = {"k": list(range(n)), "s": ["%d" % ((j * 13) % 90) if j % 9 else "n/a" for j in range(n)], "d": [None] * n, "i": [0] * n}
    ids = ref.parse(left_t["s"], "Int64", try_cast=True)
    rcols = [("rid", "Int64"), ("name", "Utf8")]
    right_t = {"rid": [3, 13, 26, 89, 1000, 26], "name": ["three", "thirteen", "twenty-six", "eighty-nine", "none", "again"]}
    lproj = projection([(c("k"), "k", "Int32"), (cast_to(c("s"), "Int64", try_cast=True), "id", "Int64")])
    inner = {"execution_plan": "hash_join_exec", "left": lproj, "right": scan(rcols), "join_type": "Inner", "mode": "CollectLeft", "on": [[c("id", lcols), c("rid", rcols)]],
             "schema": _fields(lcols + rcols)}
    want = [(j, ids[j], rid, nm) for j in range(n) for rid, nm in zip(right_t["rid"], right_t["name"]) if ids[j] == rid]
    assert sorted(_rows(run(gpu, inner, [(left_t, COLS, 2), (right_t, rcols, 1)])), key=repr) == sorted(want, key=repr) and len(want) > 10
    semi = dict(inner, join_type="Semi", schema=_fields(lcols))
    assert sorted(_rows(run(gpu, semi, [(left_t, COLS, 1), (right_t, rcols, 1)]))) == sorted((j, ids[j]) for j in range(n) if ids[j] in set(right_t["rid"]))


@pytest.mark.gpu
def test_the_fixture_end_to_end_and_split_into_stages(gpu):
    from flock_amd.runtime import ExecutionContext, collect
    from flock_amd.stages import StagedRun, build_query_dag
    n = 20_000
    cards = ["%04d %04d %04d %04d" % ((j * j) % 50 * 199, j % 10_000, 0, j % 3) for j in range(n)]
    person = pa.record_batch([pa.array(cards, pa.string())], names=["credit_card"])
    raw = open(os.path.join(PLANS, "person_card_prefix.json")).read()
    want = {}
    for s in cards:
        want[int(s[:4])] = want.get(int(s[:4]), 0) + 1
    ctx = ExecutionContext([raw], gpu=gpu)
    try:
        rb = collect(ctx, [[[person.slice(0, 7000), person.slice(7000)]]])[0][0]
    finally:
        ctx.close()
    assert rb.schema.names == ["prefix", "COUNT(UInt8(1))"] and rb.column(0).type == pa.int32()
    assert sorted(_rows(rb)) == sorted(want.items()) and len(want) > 20
    staged = StagedRun(gpu, build_query_dag(json.loads(raw)), instances=1, on_device=True)
    try:
        out = staged.run({"person": person})
    finally:
        staged.close()
    rows = []
    for b in out:
        rows += _rows(b)
    assert sorted(rows) == sorted(want.items())
