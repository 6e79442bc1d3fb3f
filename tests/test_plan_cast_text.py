"""CAST(x AS Utf8) / TRY_CAST(x AS Utf8) of Int32, Int64, UInt64 and Timestamp(ms) values (flock_amd/csrc/numtext.hpp A-NT1..A-NT7): as projected columns,
CASE branches, the value under slice functions, GROUP BY / ORDER BY / DISTINCT keys and COUNT(DISTINCT) arguments, over filters, under joins and unions and
in stage plans.  Every GPU comparison is exact -- offsets, bytes and validity -- against tests/cast_text_ref.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import cast_text_ref as ref
import scalar_fn_ref as sref
from cast_text_ref import TS, TS_MAX, TS_MIN, cast_utf8
from scalar_fn_ref import fn
from text_expr_ref import case, lit_null, lit_utf8
from text_slice_ref import lit, sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")

TILE = 1024          # textsel.hpp kTextTile: rows of a workgroup of the length and emit kernels
FLAG_TILE = 8192     # scan.hpp kFlagTile: rows of a workgroup of the general evaluator (a computed operand)

COLS = [("k", "Int32"), ("i", "Int32"), ("l", "Int64"), ("u", "UInt64"), ("t", TS), ("w", TS), ("s", "Utf8")]
TYPES = dict(COLS)


def _pa(ty):
    return pa.timestamp("ms") if ty == TS else {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string()}[ty]


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


def left(e, n):
    return sl("left", e, lit("Int64", n))


def right(e, n):
    return sl("right", e, lit("Int64", n))


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


def group_by(key_expr, parts=None, key="label"):
    """SELECT <key>, COUNT(*) GROUP BY 1 -- Partial / [Hash] / Final."""
    aggs = [{"aggregate_expr": "count", "name": "COUNT(UInt8(1))", "data_type": "UInt64", "nullable": True, "expr": lit("UInt8", 1)}]
    ins = {"fields": [_field(n, t) for n, t in COLS], "metadata": {}}
    kc = {"physical_expr": "column", "name": key, "index": 0}
    partial = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [[key_expr, key]], "aggr_expr": aggs, "input": scan(), "input_schema": ins,
               "schema": {"fields": [_field(key, "Utf8"), _field("COUNT(UInt8(1))[count]", "UInt64")], "metadata": {}}}
    mid = partial
    if parts:
        mid = {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096,
               "input": {"execution_plan": "repartition_exec", "input": partial, "partitioning": {"Hash": [[kc], parts]}}}
    return {"execution_plan": "hash_aggregate_exec", "mode": "FinalPartitioned" if parts else "Final", "group_expr": [[kc, key]], "aggr_expr": aggs, "input": mid, "input_schema": ins,
            "schema": {"fields": [_field(key, "Utf8"), _field("COUNT(UInt8(1))", "UInt64")], "metadata": {}}}


def distinct(key_expr, key="x"):
    ins = {"fields": [_field(n, t) for n, t in COLS], "metadata": {}}
    out = {"fields": [_field(key, "Utf8")], "metadata": {}}
    kc = {"physical_expr": "column", "name": key, "index": 0}
    part = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [[key_expr, key]], "aggr_expr": [], "input": scan(), "input_schema": ins, "schema": out}
    rep = {"execution_plan": "repartition_exec", "input": part, "partitioning": {"Hash": [[kc], 4]}}
    return {"execution_plan": "hash_aggregate_exec", "mode": "FinalPartitioned", "group_expr": [[kc, key]], "aggr_expr": [], "input": rep, "input_schema": ins, "schema": out}


def count_distinct(arg):
    entries = [{"aggregate_expr": "distinct_count", "name": "COUNT(DISTINCT x)", "data_type": "UInt64", "nullable": True, "exprs": [arg], "state_data_types": ["Utf8"], "input_data_types": ["Utf8"]},
               {"aggregate_expr": "count", "name": "COUNT(x)", "data_type": "UInt64", "nullable": True, "expr": lit("UInt8", 1)}]
    ins = {"fields": [_field(n, t) for n, t in COLS], "metadata": {}}
    partial = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [], "aggr_expr": entries, "input": scan(), "input_schema": ins, "schema": {"fields": [], "metadata": {}}}
    return {"execution_plan": "hash_aggregate_exec", "mode": "Final", "group_expr": [], "aggr_expr": entries, "input": {"execution_plan": "coalesce_partitions_exec", "input": partial},
            "input_schema": ins, "schema": {"fields": [_field("COUNT(DISTINCT x)", "UInt64"), _field("COUNT(x)", "UInt64")], "metadata": {}}}


# ------------------------------------------------------------------ the values
def _powers(limit):
    """0, 10^k - 1 and 10^k for every k whose 10^k is within `limit`."""
    out, p = [0], 10
    while p <= limit:
        out += [p - 1, p]
        p *= 10
    return out


I32_VALUES = sorted({s * v for v in _powers(2**31 - 1) for s in (1, -1)} | {2**31 - 1, -2**31})
I64_VALUES = sorted({s * v for v in _powers(2**63 - 1) for s in (1, -1)} | {2**63 - 1, -2**63})
U64_VALUES = sorted(set(_powers(2**64 - 1)) | {2**63, 2**64 - 1, 2**63 - 1})
DAY = 86_400_000
LEAP_DAY = 1_456_704_000_000        # 2016-02-29 00:00:00
# zero and non-zero millisecond parts (.001 .010 .100 .999), -1, the leap day, both edges of the range, moments either side of midnight and of a whole second
TS_VALUES = [0, 1, 10, 100, 999, 1000, -1, -1000, -999, LEAP_DAY, LEAP_DAY - 1, LEAP_DAY + DAY - 1, LEAP_DAY + DAY, TS_MIN, TS_MIN + 1, TS_MAX, TS_MAX - 999,
             1_700_000_000_000, 1_700_000_000_010, 1_700_000_000_100, 1_700_000_000_999, 951_782_400_000, 4_107_542_399_999, -2_208_988_800_000]
TS_BEYOND = [TS_MIN - 1, TS_MAX + 1, -2**63, 2**63 - 1]


def make_table(n):
    """Every special value of every type occurs (n >= 200); NULLs at every tile's first and last row; `w` also holds timestamps beyond the range."""
    wide = TS_VALUES + TS_BEYOND
    t = {"k": list(range(n)),
         "i": [I32_VALUES[j % len(I32_VALUES)] for j in range(n)],
         "l": [I64_VALUES[(j * 7) % len(I64_VALUES)] for j in range(n)],
         "u": [U64_VALUES[(j * 5) % len(U64_VALUES)] for j in range(n)],
         "t": [TS_VALUES[(j * 5) % len(TS_VALUES)] for j in range(n)],
         "w": [wide[(j * 3) % len(wide)] for j in range(n)],
         "s": ["s%d" % (j % 11) for j in range(n)]}
    for j in range(n):
        if j % TILE in (0, TILE - 1) or j % 97 == 5:
            for name in ("i", "l", "u", "t", "w"):
                if (j + len(name) + ord(name[0])) % 3:   # (not every column at once: a NULL beside values)
                    t[name][j] = None
            if j % TILE in (0, TILE - 1):
                t["i"][j] = t["t"][j] = None
    if n >= 200:
        for name, vals in (("i", I32_VALUES), ("l", I64_VALUES), ("u", U64_VALUES), ("t", TS_VALUES), ("w", wide)):
            assert set(vals) <= set(t[name]), (name, n, sorted(set(vals) - set(t[name]))[:4])
    return t


_TABLES = {}


def shared_table(n):
    if n not in _TABLES:
        _TABLES[n] = make_table(n)
    return _TABLES[n]


def batch(t, a, b, cols=COLS):
    return pa.record_batch([pa.array(t[cn][a:b], pa.int64()).cast(_pa(ty)) if ty == TS else pa.array(t[cn][a:b], _pa(ty)) for cn, ty in cols], names=[cn for cn, _ in cols])


def batches(t, parts, cols=COLS):
    """The table in `parts` batches of (almost) equal size."""
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


Q10_DATE = left(cast_utf8(c("t")), 10)
Q10_TIME = right(left(cast_utf8(c("t")), 16), 5)
EVERY = [cast_utf8(c("i")), cast_utf8(c("l")), cast_utf8(c("u")), cast_utf8(c("t")), cast_utf8(c("w"), try_cast=True), cast_utf8(c("l"), try_cast=True)]


# ------------------------------------------------------------------ CPU: the reference
def test_reference_by_hand():
    assert ref.int_text([0, -1, 2**63 - 1, -2**63, 2**64 - 1, None]) == ["0", "-1", "9223372036854775807", "-9223372036854775808", "18446744073709551615", None]
    assert ref.ts_text([0, -1, 1, 1000, LEAP_DAY, None]) == ["1970-01-01 00:00:00", "1969-12-31 23:59:59.999", "1970-01-01 00:00:00.001", "1970-01-01 00:00:01", "2016-02-29 00:00:00", None]
    assert ref.ts_text([TS_MIN, TS_MAX, 10, 100]) == ["0000-01-01 00:00:00", "9999-12-31 23:59:59.999", "1970-01-01 00:00:00.010", "1970-01-01 00:00:00.100"]
    assert ref.ts_text([TS_MIN - 1, TS_MAX + 1, 5], try_cast=True) == [None, None, "1970-01-01 00:00:00.005"]
    for v in (TS_MIN - 1, TS_MAX + 1):
        with pytest.raises(ref.CastRangeError):
            ref.ts_text([0, v])
    t = {"i": [5, None, -30], "t": [LEAP_DAY + 3_600_000 * 13 + 60_000 * 7, None, -1], "s": ["a", "b", None]}
    ty = {"i": "Int32", "t": TS, "s": "Utf8"}
    cc = lambda n: c(n, [("i", "Int32"), ("t", TS), ("s", "Utf8")])
    assert ref.eval_text(cast_utf8(cc("i")), t, ty) == ["5", None, "-30"]
    assert ref.eval_text(left(cast_utf8(cc("t")), 10), t, ty) == ["2016-02-29", None, "1969-12-31"]
    assert ref.eval_text(right(left(cast_utf8(cc("t")), 16), 5), t, ty) == ["13:07", None, "23:59"]
    assert ref.eval_text(cast_utf8(binary(cc("i"), "Multiply", lit("Int32", 2))), t, ty) == ["10", None, "-60"]
    assert ref.eval_text(case([(binary(cc("i"), "Gt", lit("Int32", 0)), cast_utf8(cc("i")))], lit_utf8("none")), t, ty) == ["5", "none", "none"]
    assert ref.eval_text(cast_utf8(cc("s")), t, ty) == ["a", "b", None]


def test_reference_against_pyarrow():
    for vals, ty in ((I32_VALUES, pa.int32()), (I64_VALUES, pa.int64()), (U64_VALUES, pa.uint64())):
        vals = vals + [None]
        assert pc.cast(pa.array(vals, ty), pa.string()).to_pylist() == ref.int_text(vals)
    r = np.random.default_rng(10)
    ms = TS_VALUES + [int(x) for x in r.integers(TS_MIN, TS_MAX, 3000)] + [int(x) * 1000 for x in r.integers(-10**9, 10**10, 500)] + [None]
    got = pc.cast(pa.array(ms, pa.int64()).cast(pa.timestamp("ms")), pa.string()).to_pylist()
    norm = lambda s: None if s is None else s[:-4] if s.endswith(".000") else s    # (pyarrow always prints the millisecond part)
    want = ref.ts_text(ms)
    assert [norm(g) for g in got] == want
    assert {len(w) for w in want if w is not None} == {19, 23}


def test_numtext_on_the_host():
    """numtext.hpp (digit counts, digit pairs, the timestamp layout) as a stand-alone host program against snprintf and a day-by-day calendar, under the
    address and undefined-behaviour sanitizers."""
    exe = os.path.join(ROOT, "tests", "cpp", "numtext_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "flock_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "numtext_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "numtext_test: ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ CPU: parsing, explain, refusals
def test_a_projected_cast_explains_as_utf8():
    from flock_amd.runtime import explain
    for e, text in ((cast_utf8(c("i")), "CAST(i AS Utf8)"), (cast_utf8(c("l")), "CAST(l AS Utf8)"), (cast_utf8(c("u")), "CAST(u AS Utf8)"), (cast_utf8(c("t")), "CAST(t AS Utf8)"),
                    (cast_utf8(c("t"), try_cast=True), "TRY_CAST(t AS Utf8)"), (cast_utf8(binary(c("i"), "Multiply", lit("Int32", 2))), "CAST(i * 2 AS Utf8)"),
                    (cast_utf8(cast_utf8(c("l"))), "CAST(l AS Utf8)")):
        first = explain(projection([(e, "x"), (c("k"), "k")])).splitlines()[0]
        assert first.startswith("Project(x = %s) [x:Utf8, k:Int32]" % text), first
    # a cast of a Utf8 column is the column, as before
    assert explain(projection([(cast_utf8(c("s")), "x")])).splitlines()[0].startswith("Project(x = s) [x:Utf8]")


def test_a_cast_in_a_case_under_slices_and_as_a_key_explains():
    from flock_amd.runtime import explain
    label = case([(binary(c("i"), "Gt", lit("Int32", 0)), cast_utf8(c("i")))], lit_utf8("none"))
    assert explain(projection([(label, "x")])).splitlines()[0].startswith("Project(x = CASE ...) [x:Utf8]")
    mixed = case([(mod("k", 4, 0), cast_utf8(c("l"))), (mod("k", 4, 1), c("s")), (mod("k", 4, 2), left(cast_utf8(c("t")), 4)), (mod("k", 4, 3), lit_null())], cast_utf8(c("t"), try_cast=True))
    assert "x:Utf8" in explain(projection([(mixed, "x")]))
    for e, text in ((Q10_DATE, "left(CAST(t AS Utf8), 10)"), (Q10_TIME, "right(left(CAST(t AS Utf8), 16), 5)"), (sl("split_part", cast_utf8(c("t")), lit("Utf8", " "), lit("Int64", 2)),
                    "split_part(CAST(t AS Utf8), ' ', 2)"), (right(cast_utf8(c("u")), 3), "right(CAST(u AS Utf8), 3)")):
        assert explain(projection([(e, "x")])).splitlines()[0].startswith("Project(x = %s) [x:Utf8]" % text)
    # sixteen sources: identical casts count once, different ones each
    many = lambda k: case([(mod("k", 100, j), cast_utf8(binary(c("i"), "Plus", lit("Int32", j)))) for j in range(k - 1)] + [(mod("k", 100, 50), cast_utf8(binary(c("i"), "Plus", lit("Int32", 0))))],
                          cast_utf8(c("l")))
    assert "x:Utf8" in explain(projection([(many(16), "x")]))
    refused(projection([(many(17), "x")]), "more than 16 distinct sources")
    txt = explain(group_by(cast_utf8(c("i")), parts=4))
    assert "Aggregate(Partial)" in txt and "#7:Utf8" in txt and "Project(#7 = CAST(i AS Utf8))" in txt, txt
    txt = explain(sort_(scan(), [(cast_utf8(c("i")), True), (c("k"), False)]))
    assert "Sort(#7 DESC, k ASC)" in txt and "Project(#7 = CAST(i AS Utf8))" in txt, txt
    assert "#7:Utf8" in explain(count_distinct(cast_utf8(c("l"))))
    assert "Project(#7 = CAST(u AS Utf8))" in explain(distinct(cast_utf8(c("u"))))


def test_the_q10_fixture_explains_and_is_no_fused_query():
    from flock_amd import _ffi, build
    from flock_amd.runtime import explain
    raw = open(os.path.join(PLANS, "q10_date_time_text.json")).read()
    txt = explain(raw)
    assert txt.splitlines()[0].startswith("Project(date = left(CAST(b_date_time AS Utf8), 10), time = right(left(CAST(b_date_time AS Utf8), 16), 5)) "
                                          "[auction:Int32, bidder:Int32, price:Int32, b_date_time:Timestamp(ms), date:Utf8, time:Utf8]"), txt
    assert "fused" not in txt
    build.build()
    lib = _ffi.load()
    got = C.c_int(-1)
    assert lib.flockgpu_plan_recognise(raw.encode(), len(raw.encode()), C.byref(got)) == _ffi.OK and got.value == 0


def test_refusals_by_name():
    fcols = COLS + [("f", "Float64")]
    ftypes = dict(fcols)
    p = lambda e: projection([(e, "x")], inp=scan(fcols), types=ftypes)
    for tag, tc in (("cast_expr: ", False), ("try_cast_expr: ", True)):
        refused(p(cast_utf8(c("f", fcols), try_cast=tc)), tag + "CAST of a Float64 value to Utf8")
        refused(p(cast_utf8(cast(c("i", fcols), "Float64"), try_cast=tc)), tag + "CAST of a Float64 value to Utf8")
        refused(p(cast_utf8(binary(c("i", fcols), "Gt", lit("Int32", 3)), try_cast=tc)), tag + "CAST of a Boolean value to Utf8")
        refused(p(cast_utf8(lit("Int32", 5), try_cast=tc)), tag + "CAST of a literal to Utf8", "a literal operand")
        refused(p(cast_utf8(lit("Float64", 1.5), try_cast=tc)), tag + "CAST of a literal to Utf8")
        refused(p(cast_utf8({"physical_expr": "literal", "value": 7}, try_cast=tc)), tag + "CAST of a literal to Utf8")
    # ... under a slice and in a CASE alike
    refused(p(left(cast_utf8(c("f", fcols)), 3)), "cast_expr: CAST of a Float64 value to Utf8")
    refused(p(case([(mod("k", 2, 0), cast_utf8(c("f", fcols)))], lit_utf8("x"))), "cast_expr: CAST of a Float64 value to Utf8")
    refused(p(case([(mod("k", 2, 0), cast_utf8(c("i", fcols)))], lit("Int32", 3))), "CASE branches of different types")


def test_what_stays_refused_keeps_its_message():
    from flock_amd import _ffi
    from flock_amd.runtime import FlockGpuError, explain
    # LIKE, char_length and octet_length take a Utf8 column only
    refused(filter_(binary(cast_utf8(c("i")), "Like", lit_utf8("1%"))), "LIKE on something that is not a Utf8 column")
    refused(projection([(fn("char_length", cast_utf8(c("i"))), "x")]), "function 'char_length'", "not a Utf8 column")
    refused(projection([(fn("octet_length", cast_utf8(c("t"))), "x")]), "function 'octet_length'", "not a Utf8 column")
    # text inside a condition or under an operator: a condition is compiled at execute, where it is refused as before (the GPU test below); create may
    # refuse it already, and then as unsupported
    cond = binary(cast_utf8(c("i")), "Eq", lit_utf8("5"))
    for plan in (filter_(cond), projection([(case([(cond, lit_utf8("five"))], lit_utf8("other")), "x")])):
        try:
            explain(plan)
        except FlockGpuError as e:
            assert e.code == _ffi.ERR_UNSUPPORTED, str(e)
    # a cast from Utf8 to a number is no text-valued expression
    refused(projection([(case([(mod("k", 2, 0), cast(c("s"), "Int32"))], lit_utf8("x")), "y")]), "CASE branches of different types")
    for f in ("min", "max"):
        agg = {"aggregate_expr": f, "name": "M", "data_type": "Utf8", "nullable": True, "expr": cast_utf8(c("i"))}
        plan = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [], "aggr_expr": [agg], "input": scan(),
                "input_schema": {"fields": [_field(n, t) for n, t in COLS], "metadata": {}}, "schema": {"fields": [_field("M[%s]" % f, "Utf8")], "metadata": {}}}
        refused(plan, f + " needs an integer column")


def test_stage_plans_with_a_cast_split_and_every_stage_explains():
    from flock_amd.runtime import explain
    from flock_amd.stages import build_query_dag, split_at_repartitions
    for plan in (group_by(cast_utf8(c("i")), parts=4), group_by(Q10_DATE, parts=4), distinct(cast_utf8(c("t"), try_cast=True))):
        for dag in (build_query_dag(plan), split_at_repartitions(plan)):
            assert len(dag) == 2
            texts = [explain(s.plan) for s in dag]
            assert any("AS Utf8)" in t for t in texts) and all("Utf8" in t for t in texts), texts


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


def raw_bytes(col):
    """(validity, offsets, data) of a Utf8 column: what 'identical' compares."""
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    offs = np.frombuffer(col.buffers()[1], dtype=np.int32)[col.offset:col.offset + len(col) + 1] if len(col) else np.zeros(1, np.int32)
    data = col.buffers()[2].to_pybytes()[int(offs[0]):int(offs[-1])] if len(col) and col.buffers()[2] is not None else b""
    return col.is_valid().to_pylist(), (offs - offs[0]).tolist(), data


def check(gpu, exprs, t, parts=1, cols=COLS, types=TYPES, want=None):
    """Projects k and every expression; each column equals the reference in validity, offsets and bytes."""
    plan = projection([(c("k", cols), "k")] + [(e, "x%d" % j) for j, e in enumerate(exprs)], inp=scan(cols), types=types)
    rb = run(gpu, plan, [(t, cols, parts)])
    n = len(t["k"])
    assert rb.num_rows == n and rb.column(0).to_pylist() == t["k"]
    for j, e in enumerate(exprs):
        w = pa.array(want[j] if want is not None else ref.eval_text(e, t, types), pa.string())
        got = rb.column(1 + j)
        assert got.type == pa.string()
        assert raw_bytes(got) == raw_bytes(w), (j, json.dumps(e)[:160], [(a, b) for a, b in zip(got.to_pylist(), w.to_pylist()) if a != b][:5])
    return rb


_WANT = {}


def wanted(n):
    """The reference's columns for EVERY over shared_table(n): computed once."""
    if n not in _WANT:
        _WANT[n] = [ref.eval_text(e, shared_table(n), TYPES) for e in EVERY]
    return _WANT[n]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, FLAG_TILE - 1, FLAG_TILE, FLAG_TILE + 1, 3 * FLAG_TILE + 5])
def test_row_counts_around_the_text_tile_and_the_flag_tile(gpu, n):
    t = shared_table(n)
    a = check(gpu, EVERY, t, parts=1, want=wanted(n))
    b = check(gpu, EVERY, t, parts=3, want=wanted(n))
    for j in range(1, a.num_columns):
        assert raw_bytes(a.column(j)) == raw_bytes(b.column(j)), j
    if n >= TILE:
        w = a.column(5).to_pylist()     # TRY_CAST(w): NULL where the input is NULL or beyond the range, a value everywhere else
        assert all((x is None) == (v is None or not TS_MIN <= v <= TS_MAX) for x, v in zip(w, t["w"]))
        assert a.column(1).null_count >= 2 * (n // TILE) and a.column(1).is_null().to_pylist()[TILE - 1] and (n == TILE or a.column(1).is_null().to_pylist()[TILE])


@pytest.mark.gpu
def test_a_timestamp_beyond_the_range_fails_the_call_by_name_and_try_cast_gives_null(gpu):
    from flock_amd import _ffi
    from flock_amd.runtime import FlockGpuError
    n = TILE + 3
    for bad in TS_BEYOND[:2]:
        t = dict(shared_table(n))
        t["t"] = list(t["t"])
        t["t"][TILE + 1] = bad
        with pytest.raises(FlockGpuError) as e:
            check(gpu, [cast_utf8(c("t"))], t)
        assert e.value.code == _ffi.ERR_INVALID and "cast_expr" in str(e.value) and "0000 to 9999" in str(e.value), str(e.value)
        with pytest.raises(FlockGpuError) as e:
            check(gpu, [Q10_DATE], t)
        assert "cast_expr" in str(e.value), str(e.value)
        rb = check(gpu, [cast_utf8(c("t"), try_cast=True), cast_utf8(c("i"))], t)
        assert rb.column(1).to_pylist()[TILE + 1] is None and rb.column(1).to_pylist()[TILE + 2] is not None
    # a NULL slot that holds such a value fails nothing
    arr = pa.array([TS_MAX + 5, 0, TS_MIN - 5], pa.int64(), mask=np.array([True, False, True])).cast(pa.timestamp("ms"))
    cols = [("k", "Int32"), ("t", TS)]
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([projection([(cast_utf8(c("t", cols)), "x")], inp=scan(cols), types=dict(cols))], gpu=gpu)
    try:
        rb = collect(ctx, [[[pa.record_batch([pa.array([0, 1, 2], pa.int32()), arr], names=["k", "t"])]]])[0][0]
    finally:
        ctx.close()
    assert rb.column(0).to_pylist() == [None, "1970-01-01 00:00:00", None]


@pytest.mark.gpu
def test_rows_of_one_byte_and_of_twenty_bytes_across_the_tile_seams(gpu):
    """Every row one byte long: a tile is 1024 bytes, its seams fall on 16-byte chunk boundaries until a NULL shifts them inside a chunk; every row twenty
    bytes long: a tile is 20480 bytes, and with the NULLs its seams fall at every phase."""
    n = 3 * TILE + 5
    t = dict(shared_table(n))
    t["i"] = [j % 10 for j in range(n)]
    t["l"] = [-(10**18) - j for j in range(n)]
    t["u"] = [10**19 + j for j in range(n)]
    rb = check(gpu, [cast_utf8(c("i")), cast_utf8(c("l")), cast_utf8(c("u"))], t)
    assert pc.sum(pc.binary_length(rb.column(1))).as_py() == n and pc.sum(pc.binary_length(rb.column(2))).as_py() == 20 * n
    for name in ("i", "l", "u"):
        t[name] = [None if j in (3, TILE + 7, 2 * TILE - 1, 2 * TILE) else v for j, v in enumerate(t[name])]
    rb = check(gpu, [cast_utf8(c("i")), cast_utf8(c("l")), cast_utf8(c("u"))], t, parts=3)
    assert pc.sum(pc.binary_length(rb.column(1))).as_py() == n - 4 and pc.sum(pc.binary_length(rb.column(3))).as_py() == 20 * (n - 4)


def small_table(n=40):
    t = {"k": list(range(n)), "i": [[7, 10, 9, -3, 0, 100, 99, None][j % 8] for j in range(n)], "l": [[-5, 2**40, None, 12][j % 4] for j in range(n)],
         "u": [[2**63, 3, None][j % 3] for j in range(n)], "t": [[LEAP_DAY + 47_220_123, -1, None, 86_399_000, 0][j % 5] for j in range(n)],
         "w": [[TS_MAX + 1, 5, None][j % 3] for j in range(n)], "s": [["a", None, "bc"][j % 3] for j in range(n)]}
    return t


@pytest.mark.gpu
def test_the_cast_in_a_case_under_slices_and_over_a_computed_operand(gpu):
    t = small_table()
    label = case([(binary(c("i"), "Gt", lit("Int32", 0)), cast_utf8(c("i"))), (binary(c("i"), "Eq", lit("Int32", 0)), lit_null())], lit_utf8("none"))
    mixed = case([(mod("k", 4, 0), cast_utf8(c("l"))), (mod("k", 4, 1), c("s")), (mod("k", 4, 2), left(cast_utf8(c("t")), 4)), (mod("k", 7, 3), cast_utf8(c("l")))],
                 cast_utf8(c("w"), try_cast=True))
    computed = [cast_utf8(binary(c("i"), "Multiply", lit("Int32", 2))), cast_utf8(binary(cast(c("i"), "Int64"), "Plus", c("l"))),
                cast_utf8(fn("date_trunc", lit_utf8("day"), c("t"))), cast_utf8(fn("date_part", lit_utf8("hour"), c("t"))), cast_utf8(cast(c("l"), "Timestamp(Millisecond, None)"))]
    rb = check(gpu, [label, mixed, Q10_DATE, Q10_TIME, right(cast_utf8(c("u")), 3), sl("split_part", cast_utf8(c("t")), lit("Utf8", " "), lit("Int64", 2))] + computed[:4], t, parts=3)
    assert rb.column(1).to_pylist()[:5] == ["7", "10", "9", "none", None] and rb.column(3).to_pylist()[:2] == ["2016-02-29", "1969-12-31"] and rb.column(4).to_pylist()[0] == "13:07"
    assert rb.column(7).to_pylist()[:3] == ["14", "20", "18"] and rb.column(9).to_pylist()[0] == "2016-02-29 00:00:00" and rb.column(10).to_pylist()[0] == "13"


def _rows(b):
    return list(zip(*[b.column(j).to_pylist() for j in range(b.num_columns)]))


@pytest.mark.gpu
def test_the_cast_as_group_by_order_by_distinct_and_count_distinct_key(gpu):
    t = small_table(60)
    n = 60
    labels = ref.eval_text(cast_utf8(c("i")), t, TYPES)
    want = {}
    for lab in labels:
        want[lab] = want.get(lab, 0) + 1
    for parts in (None, 4):
        assert sorted(_rows(run(gpu, group_by(cast_utf8(c("i")), parts=parts), [(t, COLS, 2)])), key=repr) == sorted(want.items(), key=repr)
    dates = ref.eval_text(Q10_DATE, t, TYPES)
    dwant = {}
    for d in dates:
        dwant[d] = dwant.get(d, 0) + 1
    assert sorted(_rows(run(gpu, group_by(Q10_DATE), [(t, COLS, 1)])), key=repr) == sorted(dwant.items(), key=repr) and len(dwant) == 4
    # ORDER BY CAST(i AS Utf8): bytewise, '10' before '9', '-3' before '0'; NULL keys last
    for desc in (False, True):
        rb = run(gpu, projection([(c("k"), "k")], sort_(scan(), [(cast_utf8(c("i")), desc), (c("k"), False)])), [(t, COLS, 1)])
        some = sorted((j for j in range(n) if labels[j] is not None), key=lambda j: (labels[j].encode(), j))
        if desc:
            some = sorted((j for j in range(n) if labels[j] is not None), key=lambda j: ([-b for b in labels[j].encode()] + [1], j))
        assert rb.column(0).to_pylist() == some + [j for j in range(n) if labels[j] is None], desc
        if not desc:
            order = [labels[j] for j in rb.column(0).to_pylist()]
            assert order.index("10") < order.index("9") and order.index("-3") < order.index("0") and order.index("100") < order.index("99")
    assert sorted(run(gpu, distinct(cast_utf8(c("u"))), [(t, COLS, 1)]).column(0).to_pylist(), key=repr) == sorted({None, str(2**63), "3"}, key=repr)
    texts = ref.eval_text(cast_utf8(c("t")), t, TYPES)
    assert _rows(run(gpu, count_distinct(cast_utf8(c("t"))), [(t, COLS, 1)])) == [(len({v for v in texts if v is not None}), n)]


@pytest.mark.gpu
def test_over_a_filter_under_a_join_and_in_a_union_branch(gpu):
    t = small_table(50)
    n = 50
    e = cast_utf8(c("i"))
    pred = binary(binary(c("k"), "Gt", lit("Int32", 5)), "And", binary(c("k"), "Lt", lit("Int32", 44)))
    keep = [5 < k < 44 for k in t["k"]]
    kept = {name: [v for v, b in zip(col, keep) if b] for name, col in t.items()}
    rb = run(gpu, projection([(c("k"), "k"), (e, "x"), (Q10_TIME, "y")], filter_(pred)), [(t, COLS, 2)])
    assert rb.column(0).to_pylist() == kept["k"]
    assert raw_bytes(rb.column(1)) == raw_bytes(pa.array(ref.eval_text(e, kept, TYPES), pa.string())) and raw_bytes(rb.column(2)) == raw_bytes(pa.array(ref.eval_text(Q10_TIME, kept, TYPES), pa.string()))
    # the projection BELOW a join: the cast is a column the join carries
    below = [("k", "Int32"), ("i", "Int32"), ("x", "Utf8")]
    lproj = projection([(c("k"), "k"), (c("i"), "i"), (cast_utf8(c("l")), "x")])
    x = ref.eval_text(cast_utf8(c("l")), t, TYPES)
    rcols = [("name", "Utf8"), ("v", "Int32")]
    right_t = {"name": ["seven", "ten", None], "v": [7, 10, 55]}
    inner = {"execution_plan": "hash_join_exec", "left": lproj, "right": scan(rcols), "join_type": "Inner", "mode": "CollectLeft", "on": [[c("i", below), c("v", rcols)]],
             "schema": {"fields": [_field(nm, ty) for nm, ty in below + rcols], "metadata": {}}}
    rb = run(gpu, inner, [(t, COLS, 1), (right_t, rcols, 1)])
    name_of = {7: "seven", 10: "ten"}
    want = [(t["k"][j], t["i"][j], x[j], name_of[t["i"][j]], t["i"][j]) for j in range(n) if t["i"][j] in name_of]
    assert sorted(_rows(rb), key=repr) == sorted(want, key=repr) and len(want) > 8
    # UNION ALL of a Utf8 column and an id made text
    out = [("k", "Int32"), ("x", "Utf8")]
    a = projection([(c("k"), "k"), (c("s"), "x")])
    b = projection([(c("k"), "k"), (cast_utf8(c("u")), "x")])
    union = {"execution_plan": "union_exec", "inputs": [a, b], "schema": {"fields": [_field(nm, ty) for nm, ty in out], "metadata": {}}}
    rb = run(gpu, union, [(t, COLS, 1), (t, COLS, 2)])
    assert sorted(_rows(rb), key=repr) == sorted(list(zip(t["k"], t["s"])) + list(zip(t["k"], ref.eval_text(cast_utf8(c("u")), t, TYPES))), key=repr)


@pytest.mark.gpu
def test_text_in_a_condition_stays_refused(gpu):
    from flock_amd import _ffi
    from flock_amd.runtime import FlockGpuError
    t = small_table(8)
    cond = binary(cast_utf8(c("i")), "Eq", lit_utf8("5"))
    for plan in (projection([(c("k"), "k")], filter_(cond)), projection([(case([(cond, lit_utf8("five"))], lit_utf8("other")), "x")])):
        with pytest.raises(FlockGpuError) as e:
            run(gpu, plan, [(t, COLS, 1)])
        assert e.value.code == _ffi.ERR_UNSUPPORTED, str(e.value)


@pytest.mark.gpu
def test_q10_end_to_end(gpu):
    """100 000 bids whose times lie either side of midnight and of a whole second, fed in chunks of 30 000."""
    from flock_amd.runtime import ExecutionContext, collect
    n = 100_000
    r = np.random.default_rng(10)
    base = 1_700_000_000_000 - 1_700_000_000_000 % DAY      # a midnight
    ms = base + r.integers(0, 3, n) * DAY + r.integers(-2000, 2001, n)      # within two seconds of a midnight
    ms[::7] = base + r.integers(0, 3 * DAY, len(ms[::7])) // 1000 * 1000 + r.choice([-1, 0, 1, 999, 500], len(ms[::7]))   # ... and around whole seconds all day
    bid_cols = [("auction", "Int32"), ("bidder", "Int32"), ("price", "Int32"), ("b_date_time", TS)]
    bid = {"auction": list(range(n)), "bidder": [j % 13 for j in range(n)], "price": [(j * 37) % 10_000 for j in range(n)], "b_date_time": [int(x) for x in ms]}
    feed = [batch(bid, a, min(a + 30_000, n), bid_cols) for a in range(0, n, 30_000)]
    ctx = ExecutionContext([open(os.path.join(PLANS, "q10_date_time_text.json")).read()], gpu=gpu)
    try:
        rb = collect(ctx, [[feed]])[0][0]
    finally:
        ctx.close()
    assert rb.schema.names == ["auction", "bidder", "price", "b_date_time", "date", "time"] and rb.num_rows == n
    text = ref.ts_text(bid["b_date_time"])
    assert rb.column(0).to_pylist() == bid["auction"] and rb.column(3).cast(pa.int64()).to_pylist() == bid["b_date_time"]
    assert raw_bytes(rb.column(4)) == raw_bytes(pa.array([s[:10] for s in text], pa.string()))
    assert raw_bytes(rb.column(5)) == raw_bytes(pa.array([s[11:16] for s in text], pa.string()))
    assert len(set(rb.column(4).to_pylist())) >= 4 and {"23:59", "00:00"} <= set(rb.column(5).to_pylist()) and {len(s) for s in text} == {19, 23}
