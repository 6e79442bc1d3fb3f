"""Utf8-valued expressions (flock_amd/csrc/textsel.hpp A-T1..A-T5): text literals, CAST(column AS Utf8) and CASE with text branches as projected columns, GROUP BY /
ORDER BY keys and COUNT(DISTINCT) arguments, over filters and joins and in stage plans.  Every GPU comparison is row for row and byte for byte against
tests/text_expr_ref.py, the input fed in several batches.

Not tested on the GPU: the refusal of a result of 2^31 bytes or more (A-T5).  A result that large does not fit a test of a few seconds; the check reads the total
the length pass publishes, before the byte buffer is sized or any byte is written."""
import ctypes as C
import json
import os

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import scalar_fn_ref as sref
import text_expr_ref as ref
from scalar_fn_ref import TS, fn
from text_expr_ref import case, lit_null, lit_utf8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")

TILE = 1024          # textsel.hpp kTextTile: rows of a workgroup of the length and emit kernels
FLAG_TILE = 8192     # scan.hpp kFlagTile: rows of a tile of the evaluator that computes the selector
STAGE = 16384        # textsel.hpp kTextStageBytes: bytes of one emit round

COLS = [("k", "Int32"), ("i", "Int32"), ("l", "Int64"), ("f", "Float64"), ("t", "ts"), ("s", "Utf8"), ("u", "Utf8")]
NAMES = [c for c, _ in COLS]
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string(), "ts": pa.timestamp("ms")}
TYPES = {c: (TS if t == "ts" else t) for c, t in COLS}
WORDS = ["", "a", "été", "€", "\U0001F600", "x" * 15, "y" * 16, "z" * 17, "w" * 70, "aé€\U0001F600"]


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


def cast(e, t):
    return {"physical_expr": "cast_expr", "expr": e, "cast_type": t}


def mod(col, m, r):
    return binary(binary(c(col), "Modulo", lit("Int32", m)), "Eq", lit("Int32", r))


def scan(cols=COLS):
    return {"execution_plan": "memory_exec", "schema": {"fields": [_field(n, t) for n, t in cols], "metadata": {}}, "projection": list(range(len(cols)))}


def projection(exprs, inp=None, out_types=None):
    """exprs: (expression, name); a computed column is Utf8 unless out_types names its type."""
    def ty(e, n):
        if out_types and n in out_types:
            return out_types[n]
        return TYPES[e["name"]] if e.get("physical_expr") == "column" and e["name"] in TYPES else "Utf8"
    return {"execution_plan": "projection_exec", "expr": [[e, n] for e, n in exprs], "input": scan() if inp is None else inp,
            "schema": {"fields": [_field(n, "x") | {"data_type": ty(e, n)} for e, n in exprs], "metadata": {}}}


def filter_(pred, inp=None):
    return {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096, "input": {"execution_plan": "filter_exec", "predicate": pred, "input": scan() if inp is None else inp}}


def sort_(inp, keys):
    return {"execution_plan": "sort_exec", "input": inp, "expr": [{"expr": e, "options": {"descending": d, "nulls_first": False}} for e, d in keys]}


def make_table(n, seed, null_p=0.15):
    r = np.random.default_rng(seed)
    nul = lambda xs: [None if r.random() < null_p else x for x in xs]
    return {"k": list(range(n)), "i": nul([int(x) for x in r.integers(-40, 400, n)]), "l": nul([int(x) for x in r.integers(-2**40, 2**40, n)]),
            "f": nul([float(x) for x in np.round(r.normal(0, 50, n), 2)]), "t": nul([int(x) for x in r.integers(1_400_000_000_000, 1_500_000_000_000, n)]),
            "s": nul([WORDS[int(x)] + ("%d" % x if x % 3 == 0 else "") for x in r.integers(0, len(WORDS), n)]),
            "u": nul(["u%d" % x for x in r.integers(0, 50, n)])}


_TABLES = {}


def shared_table(n, null_p=0.15):
    if (n, null_p) not in _TABLES:
        _TABLES[(n, null_p)] = make_table(n, 300 + n, null_p)
    return _TABLES[(n, null_p)]


def batches(t, chunk, cols=COLS):
    n = len(t[cols[0][0]])
    return [pa.record_batch([pa.array(t[cn][a:a + chunk], _PA[ty]) for cn, ty in cols], names=[cn for cn, _ in cols]) for a in range(0, max(n, 1), max(chunk, 1))]


def mixed_case():
    """Literals, both Utf8 columns, a NULL branch, a nested CASE, conditions with NULLs -- no ELSE."""
    inner = case([(binary(c("f"), "Gt", lit("Float64", 0.0)), c("u"))], lit_utf8("nested-else"))
    return case([(mod("i", 5, 0), lit_utf8("five")), (binary(c("l"), "Lt", lit("Int64", 0)), c("s")), (mod("i", 5, 1), lit_null()), (mod("i", 5, 2), inner),
                 (mod("i", 5, 3), lit_utf8(""))])


def refused(plan, *words):
    from flock_amd import _ffi
    from flock_amd.runtime import FlockGpuError, explain
    with pytest.raises(FlockGpuError) as e:
        explain(plan)
    assert e.value.code == _ffi.ERR_UNSUPPORTED, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


# ------------------------------------------------------------------ CPU: the reference
def test_reference_by_hand():
    t = {"i": [1, 2, 3, None, 5, 6], "s": ["a", None, "", "d", "e", "f"], "u": ["U", "V", "W", "X", None, "Z"]}
    ty = {"i": "Int32", "s": "Utf8", "u": "Utf8"}
    ci = {"physical_expr": "column", "name": "i", "index": 0}
    cs = {"physical_expr": "column", "name": "s", "index": 1}
    cu = {"physical_expr": "column", "name": "u", "index": 2}
    gt = lambda v: binary(ci, "Gt", lit("Int32", v))
    # the first TRUE wins; a NULL condition is not true; ELSE
    assert ref.eval_text(case([(gt(4), lit_utf8("big")), (gt(1), lit_utf8("mid"))], lit_utf8("small")), t, ty) == ["small", "mid", "mid", "small", "big", "big"]
    # no ELSE: NULL; a NULL THEN; '' is a value
    assert ref.eval_text(case([(gt(4), lit_null()), (gt(2), lit_utf8(""))]), t, ty) == [None, None, "", None, None, None]
    assert ref.eval_text(case([(gt(2), lit_null("Utf8"))], lit_utf8("x")), t, ty) == ["x", "x", None, "x", None, None]
    # column sources: a NULL in the chosen column is NULL, the other column's NULL does not matter
    assert ref.eval_text(case([(gt(1), cs)], cu), t, ty) == ["U", None, "", "X", "e", "f"]
    # the base form: i = 2, i = 5; a NULL base matches nothing
    assert ref.eval_text(case([(lit("Int32", 2), lit_utf8("two")), (lit("Int32", 5), cs)], lit_utf8("-"), base=ci), t, ty) == ["-", "two", "-", "-", "e", "-"]
    # nested
    inner = case([(gt(5), lit_utf8("six"))], cu)
    assert ref.eval_text(case([(gt(3), inner)], lit_utf8("low")), t, ty) == ["low", "low", "low", "low", None, "six"]
    # bare forms
    assert ref.eval_text(lit_utf8("bid"), t, ty) == ["bid"] * 6 and ref.eval_text(cast(cs, "Utf8"), t, ty) == t["s"] and ref.eval_text(lit_null("Utf8"), t, ty) == [None] * 6
    with pytest.raises(ref.TextExprError):
        ref.eval_text(case([(gt(1), lit_utf8("a"))], lit("Int32", 3)), t, ty)
    assert ref.is_text(case([(gt(1), lit_null())], lit_utf8("x")), ty) is True and ref.is_text(case([(gt(1), lit_null())]), ty) is False


def test_pyarrow_takes_a_null_condition_as_not_true():
    conds = pa.StructArray.from_arrays([pa.array([True, None, False, None])], names=["c0"])
    assert pc.case_when(conds, pa.scalar("lit", pa.string())).to_pylist() == ["lit", None, None, None]


@pytest.mark.parametrize("seed", range(4))
def test_reference_against_pyarrow_case_when(seed):
    r = np.random.default_rng(70 + seed)
    n = 2000
    t = make_table(n, 900 + seed, null_p=0.3)
    conds_e = [binary(c("i"), "Gt", lit("Int32", int(r.integers(0, 300)))), binary(c("f"), "Lt", lit("Float64", float(r.integers(-30, 30)))), mod("i", 3, int(r.integers(0, 3)))]
    values_e = [lit_utf8("lit-%d" % seed), c("s"), c("u")]
    r.shuffle(values_e)
    els = [None, lit_utf8(""), c("u"), lit_null("Utf8")][seed]
    got = ref.eval_text(case(list(zip(conds_e, values_e)), els), t, TYPES)
    conds = [sref.eval_rows(e, t, TYPES, want="Boolean") for e in conds_e]
    assert any(v is None for cl in conds for v in cl)
    as_arrow = lambda e: pa.array(ref.eval_text(e, t, TYPES), pa.string())
    args = [as_arrow(v) for v in values_e] + ([as_arrow(els)] if els is not None else [])
    want = pc.case_when(pa.StructArray.from_arrays([pa.array(cl, pa.bool_()) for cl in conds], names=["c0", "c1", "c2"]), *args).to_pylist()
    assert got == want and any(v is None for v in got) and any(v == "" for v in got) is (seed == 1 or "" in got)


# ------------------------------------------------------------------ CPU: parsing, explain, refusals
def _group_by_text(key_expr, parts=None, key="label"):
    """SELECT <text CASE>, COUNT(*), SUM(i), COUNT(<text CASE>) GROUP BY 1 -- Partial / [Hash] / Final."""
    aggs = [{"aggregate_expr": "count", "name": "COUNT(UInt8(1))", "data_type": "UInt64", "nullable": True, "expr": lit("UInt8", 1)},
            {"aggregate_expr": "sum", "name": "SUM(i)", "data_type": "Int64", "nullable": True, "expr": c("i")},
            {"aggregate_expr": "count", "name": "COUNT(label)", "data_type": "UInt64", "nullable": True, "expr": key_expr}]
    ins = {"fields": [_field(n, t) for n, t in COLS], "metadata": {}}
    partial = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [[key_expr, key]], "aggr_expr": aggs, "input": scan(), "input_schema": ins,
               "schema": {"fields": [_field(key, "Utf8"), _field("COUNT(UInt8(1))[count]", "UInt64"), _field("SUM(i)[sum]", "Int64"), _field("COUNT(label)[count]", "UInt64")], "metadata": {}}}
    mid = partial
    if parts:
        mid = {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096,
               "input": {"execution_plan": "repartition_exec", "input": partial, "partitioning": {"Hash": [[{"physical_expr": "column", "name": key, "index": 0}], parts]}}}
    return {"execution_plan": "hash_aggregate_exec", "mode": "FinalPartitioned" if parts else "Final", "group_expr": [[{"physical_expr": "column", "name": key, "index": 0}, key]],
            "aggr_expr": aggs, "input": mid, "input_schema": ins,
            "schema": {"fields": [_field(key, "Utf8"), _field("COUNT(UInt8(1))", "UInt64"), _field("SUM(i)", "Int64"), _field("COUNT(label)", "UInt64")], "metadata": {}}}


def _count_distinct(arg):
    """SELECT COUNT(DISTINCT <arg>), COUNT(*) -- ungrouped, Partial / Final read as one pass."""
    entries = [{"aggregate_expr": "distinct_count", "name": "COUNT(DISTINCT x)", "data_type": "UInt64", "nullable": True, "exprs": [arg], "state_data_types": ["Utf8"], "input_data_types": ["Utf8"]},
               {"aggregate_expr": "count", "name": "COUNT(x)", "data_type": "UInt64", "nullable": True, "expr": lit("UInt8", 1)}]
    ins = {"fields": [_field(n, t) for n, t in COLS], "metadata": {}}
    partial = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [], "aggr_expr": entries, "input": scan(), "input_schema": ins, "schema": {"fields": [], "metadata": {}}}
    return {"execution_plan": "hash_aggregate_exec", "mode": "Final", "group_expr": [], "aggr_expr": entries, "input": {"execution_plan": "coalesce_partitions_exec", "input": partial},
            "input_schema": ins, "schema": {"fields": [_field("COUNT(DISTINCT x)", "UInt64"), _field("COUNT(x)", "UInt64")], "metadata": {}}}


LOW_HIGH = case([(binary(c("i"), "Lt", lit("Int32", 100)), lit_utf8("low"))], lit_utf8("high"))


def test_explain_shows_a_utf8_column_for_every_form():
    from flock_amd.runtime import explain
    first = explain(projection([(lit_utf8("bid"), "x"), (c("k"), "k")])).splitlines()[0]
    assert first.startswith("Project(x = 'bid') [x:Utf8, k:Int32]"), first
    first = explain(projection([(LOW_HIGH, "x")])).splitlines()[0]
    assert first.startswith("Project(x = CASE ...) [x:Utf8]"), first
    # a code point above U+FFFF arrives as a \\u surrogate pair and is one code point of four bytes
    assert "\\ud83d\\ude00" in json.dumps(lit_utf8("\U0001F600")) and "Project(x = 'é€\U0001F600')" in explain(projection([(lit_utf8("é€\U0001F600"), "x")]))
    for e in (cast(c("s"), "Utf8"), lit_null("Utf8"), case([(mod("i", 2, 0), c("s"))], c("u")), case([(lit("Int32", 3), lit_utf8("three"))], base=c("i")),
              case([(mod("i", 2, 0), lit_null()), (mod("i", 2, 1), lit_null())], lit_utf8("x")),           # the type is found behind leading NULL branches
              case([(mod("i", 2, 0), case([(mod("i", 3, 0), c("s"))], lit_utf8("in")))])):
        assert "x:Utf8" in explain(projection([(e, "x")])).splitlines()[0], json.dumps(e)
    txt = explain(_group_by_text(LOW_HIGH, parts=4))
    assert "Aggregate(Partial)" in txt and "#7:Utf8" in txt and "Project(#7 = CASE ..., #8 = CASE ...)" in txt, txt      # (the key, and COUNT's argument)
    assert txt.splitlines()[0].startswith("Aggregate(FinalPartitioned) [label:Utf8, "), txt
    txt = explain(sort_(scan(), [(LOW_HIGH, False), (c("k"), False)]))
    lines = txt.splitlines()
    assert lines[0].startswith("Project [k:Int32") and "#7" not in lines[0] and lines[1].strip().startswith("Sort(#7 ASC, k ASC)") and "Project(#7 = CASE ...)" in lines[2], txt
    assert "#7:Utf8" in explain(_count_distinct(LOW_HIGH))


def test_the_scan_under_a_text_case_reads_the_source_and_condition_columns_only():
    """The right input of a semi join is read for its keys alone, and its scan says what it uploads: the key is the text CASE, so the scan reads the CASE's
    columns -- conditions i and f, sources s and u -- and nothing else."""
    from flock_amd.runtime import explain
    e = case([(mod("i", 2, 0), c("s")), (binary(c("f"), "Gt", lit("Float64", 0.0)), lit_utf8("pos"))], c("u"))
    right = projection([(e, "x"), (c("l"), "l")])
    lcols = [("ls", "Utf8"), ("lk", "Int32")]
    plan = {"execution_plan": "hash_join_exec", "left": scan(lcols), "right": right, "join_type": "Semi", "mode": "CollectLeft",
            "on": [[c("ls", lcols), {"physical_expr": "column", "name": "x", "index": 0}]], "schema": {"fields": [_field(n, t) for n, t in lcols], "metadata": {}}}
    txt = explain(plan)
    assert "reads [i, f, s, u]" in txt, txt


def test_the_limits_of_one_expression_are_refused_by_name():
    from flock_amd.runtime import explain
    many = lambda k: case([(mod("i", 100, j), lit_utf8("v%d" % j)) for j in range(k - 1)], lit_utf8("else"))
    assert "x:Utf8" in explain(projection([(many(16), "x")]))
    refused(projection([(many(17), "x")]), "more than 16 distinct sources")
    # fourteen literals and both columns are 16; one more literal is 17; a repeated literal or column counts once
    with_cols = lambda k: case([(mod("i", 100, j), lit_utf8("v%d" % j)) for j in range(k)] + [(mod("i", 100, 50), c("s")), (mod("i", 100, 51), c("s"))], c("u"))
    assert "x:Utf8" in explain(projection([(with_cols(14), "x")]))
    refused(projection([(with_cols(15), "x")]), "more than 16 distinct sources")
    assert "x:Utf8" in explain(projection([(case([(mod("i", 100, j), lit_utf8("same")) for j in range(40)]), "x")]))
    big = lambda n: case([(mod("i", 2, 0), lit_utf8("a" * 512))], lit_utf8("b" * (n - 512)))
    assert "x:Utf8" in explain(projection([(big(1024), "x")]))
    refused(projection([(big(1025), "x")]), "more than 1024 bytes of literals")
    refused(_group_by_text(many(17)), "more than 16 distinct sources")
    refused(sort_(scan(), [(big(1025), False)]), "more than 1024 bytes of literals")


def test_what_stays_refused_keeps_its_message():
    from flock_amd import GpuContext  # noqa: F401  (the package imports without a GPU)
    from flock_amd.runtime import FlockGpuError, explain
    # text beside numbers in one CASE, whichever comes first
    refused(projection([(case([(mod("i", 2, 0), lit_utf8("a"))], lit("Int32", 3)), "x")]), "CASE branches of different types")
    refused(projection([(case([(mod("i", 2, 0), lit("Int32", 3))], lit_utf8("a")), "x")], out_types={"x": "Int32"}), "CASE branches of different types")
    refused(projection([(case([(mod("i", 2, 0), c("s"))], c("i")), "x")]), "CASE branches of different types")
    # the -2 case keeps its words
    refused(projection([(binary(c("i"), "Plus", c("l")), "x")], out_types={"x": "Int64"}), "without a numeric type")
    refused(_group_by_text(binary(c("i"), "Plus", c("l"))), "GROUP BY over an expression without a numeric type")
    # LIKE inside a computed expression; text-producing functions; a Boolean projection; hash partitioning on an expression
    like = binary(c("s"), "Like", lit_utf8("a%"))
    refused(projection([(case([(like, lit_utf8("a"))], lit_utf8("b")), "x")]), "LIKE inside a computed expression")
    refused(projection([(fn("lower", c("s")), "x")]), "'lower'", "produces text: not yet")
    refused(projection([(case([(mod("i", 2, 0), fn("upper", c("s")))], lit_utf8("b")), "x")]), "'upper'", "produces text: not yet")
    refused(projection([(binary(LOW_HIGH, "Eq", lit_utf8("low")), "x")]), "Boolean")
    refused(projection([(binary(c("s"), "Eq", lit_utf8("low")), "x")]), "Boolean")
    refused({"execution_plan": "repartition_exec", "input": scan(), "partitioning": {"Hash": [[LOW_HIGH], 4]}}, "Hash partitioning on a computed expression")
    # MIN / MAX of text
    for f in ("min", "max"):
        agg = {"aggregate_expr": f, "name": "M", "data_type": "Utf8", "nullable": True, "expr": LOW_HIGH}
        plan = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [], "aggr_expr": [agg], "input": scan(),
                "input_schema": {"fields": [_field(n, t) for n, t in COLS], "metadata": {}}, "schema": {"fields": [_field("M[%s]" % f, "Utf8")], "metadata": {}}}
        refused(plan, f + " needs an integer column")
    # a Utf8 column or literal inside a condition or under an operator passes create as before (the type of the CASE is numeric / text) and is refused when the
    # evaluator meets it: the GPU half pins the messages (test_text_inside_a_condition_is_refused_at_execute)
    assert "x:Int32" in explain(projection([(case([(binary(c("s"), "Eq", lit_utf8("or")), lit("Int32", 1))], lit("Int32", 0)), "x")], out_types={"x": "Int32"}))


def test_q14_explains_and_is_not_a_fused_query():
    from flock_amd import _ffi, build
    from flock_amd.runtime import explain
    raw = open(os.path.join(PLANS, "q14_bid_time_type.json")).read()
    txt = explain(raw)
    first = txt.splitlines()[0]
    assert first.startswith("Project(bid_time_type = CASE ...) [auction:Int32, bidder:Int32, price:Float64, bid_time_type:Utf8, b_date_time:Timestamp(ms)]"), txt
    assert "Filter" in txt and "Scan(bid)" in txt and "fused" not in txt, txt
    build.build()
    lib = _ffi.load()
    got = C.c_int(-1)
    assert lib.flockgpu_plan_recognise(raw.encode(), len(raw.encode()), C.byref(got)) == _ffi.OK and got.value == 0


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


def check_text(gpu, exprs, t, chunk=7_000, srcs=None):
    """Projects k and every expression; each column equals the reference value for value, NULLs as NULLs, '' as ''."""
    plan = projection([(c("k"), "k")] + [(e, "x%d" % j) for j, e in enumerate(exprs)])
    rb = run(gpu, plan, [(srcs if srcs is not None else t, COLS)], chunk)
    n = len(t["k"])
    assert rb.num_rows == n and rb.column(0).to_pylist() == t["k"]
    for j, e in enumerate(exprs):
        want = pa.array(ref.eval_text(e, t, TYPES), pa.string())
        got = rb.column(1 + j)
        assert got.type == pa.string()
        assert got.equals(want), (j, [(a, b) for a, b in zip(got.to_pylist(), want.to_pylist()) if a != b][:5])
    return rb


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, FLAG_TILE - 1, FLAG_TILE, FLAG_TILE + 1, 3 * FLAG_TILE + 5])
def test_row_counts_around_the_tiles(gpu, n):
    t = shared_table(n)
    check_text(gpu, [mixed_case(), LOW_HIGH, lit_utf8("bid"), cast(c("s"), "Utf8"), lit_null("Utf8"), lit_utf8("")], t, chunk=max(n // 3, 1) + 1)


@pytest.mark.gpu
def test_two_hundred_tiles_and_a_row(gpu):
    """200 tiles of the evaluator (1600 of the text kernels) and one row; the reference's picking over conditions computed with numpy."""
    n = 200 * FLAG_TILE + 1
    i = np.arange(n, dtype=np.int64) * 7 % 1000
    s = ["s%d" % v for v in (i % 97).tolist()]
    t = {"k": np.arange(n, dtype=np.int32), "i": i.astype(np.int32), "s": s}
    cols = [("k", "Int32"), ("i", "Int32"), ("s", "Utf8")]
    e = case([(binary(binary(c("i", cols), "Modulo", lit("Int32", 3)), "Eq", lit("Int32", 0)), lit_utf8("three")),
              (binary(binary(c("i", cols), "Modulo", lit("Int32", 3)), "Eq", lit("Int32", 1)), c("s", cols))])
    conds = [(i % 3 == 0).tolist(), (i % 3 == 1).tolist()]
    want = pa.array(ref.pick(conds, [["three"] * n, s], None, n), pa.string())
    whole = pa.record_batch([pa.array(t["k"]), pa.array(t["i"]), pa.array(s, pa.string())], names=["k", "i", "s"])
    bs = [whole.slice(a, 500_000) for a in range(0, n, 500_000)]
    plan = {"execution_plan": "projection_exec", "expr": [[e, "x"]], "input": scan(cols), "schema": {"fields": [_field("x", "Utf8")], "metadata": {}}}
    rb = run(gpu, plan, [(bs, cols)])
    assert rb.num_rows == n and rb.column(0).equals(want)


@pytest.mark.gpu
def test_all_null_all_empty_and_a_tile_without_bytes(gpu):
    n = 3 * TILE + 7
    t = dict(shared_table(n))
    never = binary(c("k"), "Lt", lit("Int32", 0))
    # every row NULL: no WHEN is true and there is no ELSE; a chosen column that is NULL everywhere
    t["u"] = [None] * n
    check_text(gpu, [case([(never, lit_utf8("x"))]), case([(never, lit_utf8("x"))], c("u")), cast(c("u"), "Utf8")], t)
    # every row '': zero bytes in total
    rb = check_text(gpu, [case([(never, lit_utf8("x"))], lit_utf8("")), lit_utf8("")], t)
    assert rb.column(1).null_count == 0 and pc.sum(pc.binary_length(rb.column(1))).as_py() == 0
    # the second tile emits nothing -- NULLs and '' -- between tiles that emit
    middle = binary(binary(c("k"), "GtEq", lit("Int32", TILE)), "And", binary(c("k"), "Lt", lit("Int32", 2 * TILE)))
    e = case([(binary(middle, "And", mod("k", 2, 0)), lit_utf8("")), (middle, lit_null())], lit_utf8("outside"))
    rb = check_text(gpu, [e, case([(middle, lit_utf8(""))], c("s"))], t)
    assert rb.column(1).slice(TILE, TILE).null_count == TILE // 2


@pytest.mark.gpu
def test_literal_lengths_and_multi_byte_text(gpu):
    lits = ["a", "abc", "x" * 15, "y" * 16, "z" * 17, "q" * 255, "été€\U0001F600", "\U0001F600" * 9, ""]
    t = shared_table(3 * TILE + 7)
    e = case([(mod("k", 10, j), lit_utf8(v)) for j, v in enumerate(lits)])
    check_text(gpu, [e] + [lit_utf8(v) for v in lits], t)


def _long_values(n, lengths):
    """Column s: values of the given byte lengths spread over the rows (the rest short), NULLs between them."""
    s = ["r%d" % j if j % 11 else None for j in range(n)]
    at = {}
    for j, ln in enumerate(lengths):
        row = 3 + j * (n // len(lengths))
        s[row] = (("%d-" % ln) + "abcdefghijklmnopqrstuvwxyz€" * (ln // 20 + 1)).encode()[:ln].decode("utf-8", "ignore")
        s[row] += "." * (ln - len(s[row].encode()))
        assert len(s[row].encode()) == ln
        at[ln] = row
    return s, at


@pytest.mark.gpu
def test_column_values_of_every_length_and_around_the_emit_stage(gpu):
    n = 2 * TILE + 9
    lengths = [0, 15, 16, 17, 70, 40_000, 200_000, STAGE - 1, STAGE, STAGE + 1, 3 * STAGE + 5]
    t = dict(shared_table(n))
    t["s"], at = _long_values(n, lengths)
    e = case([(mod("k", 4, 0), lit_utf8("lit"))], c("s"))          # rows 3 + j * (n // 11): a long value is taken where k % 4 != 0
    for ln, row in at.items():
        if row % 4 == 0:
            t["s"][row], t["s"][row + 1] = t["s"][row + 1], t["s"][row]
            at[ln] = row + 1
    rb = check_text(gpu, [e, cast(c("s"), "Utf8"), case([(mod("k", 2, 0), c("s"))], c("u"))], t, chunk=900)
    lens = pc.binary_length(rb.column(1)).to_pylist()
    assert [lens[at[ln]] for ln in lengths] == lengths


@pytest.mark.gpu
def test_a_sliced_source_column_and_sixteen_sources(gpu):
    n = 2 * TILE + 5
    t = shared_table(n)
    # The batches are slices of one array: the second and third begin at byte offsets that are neither 0 nor multiples of 4.  The feed rebases every
    # batch's offsets onto the column's byte cursor, so what this exercises is the FEED of such slices under a text CASE: the kernels see one
    # concatenated column whose first offset is 0 (no plan path hands them a column view with another first offset: takes and feeds both start at
    # 0).  Value start addresses inside the column are arbitrary in every test here, which is what the kernels' misaligned source reads depend on.
    whole = pa.record_batch([pa.array(t[cn], _PA[ty]) for cn, ty in COLS], names=NAMES)
    cuts = [0, 701, 1502, n]
    offs = whole.column(NAMES.index("s")).buffers()[1]
    raw = np.frombuffer(offs, dtype=np.int32)
    assert any(raw[a] % 4 not in (0,) and raw[a] > 0 for a in cuts[1:3])
    bs = [whole.slice(a, b - a) for a, b in zip(cuts, cuts[1:])]
    check_text(gpu, [mixed_case(), case([(mod("k", 3, 0), c("s"))], c("u"))], t, srcs=bs)
    # sixteen sources: thirteen literals, both columns, the ELSE.  The selector is ONE program of the evaluator (32 constants, a division by a literal
    # takes four): the conditions compare a column with the very numbers the sources are indexed by, so the program holds sixteen constants
    t16 = dict(t)
    t16["i"] = [None if j % 23 == 0 else j % 20 for j in range(n)]
    eq = lambda j: binary(c("i"), "Eq", lit("Int32", j))
    sixteen = case([(eq(j), lit_utf8("v%d" % j * (j + 1))) for j in range(13)] + [(eq(13), c("s")), (eq(14), c("u"))], lit_utf8("else"))
    rb = check_text(gpu, [sixteen], t16)
    assert len(set(rb.column(1).to_pylist())) > 16


@pytest.mark.gpu
def test_over_a_filter_an_inner_join_and_a_semi_join(gpu):
    n = FLAG_TILE + 1
    left = shared_table(n)
    pred = binary(binary(c("i"), "Gt", lit("Int32", 50)), "And", binary(c("f"), "Lt", lit("Float64", 40.0)))
    keep = sref.eval_rows(pred, left, TYPES, want="Boolean")
    kept = {name: [v for v, b in zip(col, keep) if b is True] for name, col in left.items()}
    assert 0 < len(kept["k"]) < n
    e = mixed_case()
    rb = run(gpu, projection([(c("k"), "k"), (e, "x")], filter_(pred)), [(left, COLS)])
    assert rb.column(0).to_pylist() == kept["k"] and rb.column(1).equals(pa.array(ref.eval_text(e, kept, TYPES), pa.string()))
    rcols = [(nm + "_r", ty) for nm, ty in COLS]
    right = {nm + "_r": v for nm, v in shared_table(2000, 0.4).items()}
    both = COLS + rcols

    def join(jt):
        return {"execution_plan": "hash_join_exec", "left": filter_(pred), "right": scan(rcols), "join_type": jt, "mode": "CollectLeft", "on": [[c("i"), c("i_r", rcols)]],
                "schema": {"fields": [_field(nm, ty) for nm, ty in (both if jt == "Inner" else COLS)], "metadata": {}}}
    rkeys = {v for v in right["i_r"] if v is not None}
    semi = run(gpu, projection([(c("k"), "k"), (e, "x")], join("Semi")), [(left, COLS), (right, rcols)])
    rows = [j for j, v in enumerate(kept["i"]) if v in rkeys]
    sk = {name: [col[j] for j in rows] for name, col in kept.items()}
    assert semi.column(0).to_pylist() == sk["k"] and semi.column(1).equals(pa.array(ref.eval_text(e, sk, TYPES), pa.string())) and len(rows) > 100
    # over the inner join the CASE reads a source of either side: s from the left, u_r from the right
    ej = case([(binary(c("k_r", both), "Gt", c("k", both)), c("u_r", both)), (mod("k", 3, 0), lit_utf8("third"))], c("s", both))
    inner = run(gpu, projection([(c("k", both), "k"), (c("k_r", both), "k_r"), (ej, "x")], join("Inner"), out_types={"k_r": "Int32"}), [(left, COLS), (right, rcols)])
    pairs = [(a, b) for a in range(len(kept["k"])) if kept["i"][a] is not None for b in range(2000) if right["i_r"][b] == kept["i"][a]]
    jt_ = {name: [kept[name][a] for a, _ in pairs] for name in NAMES}
    jt_.update({name: [right[name][b] for _, b in pairs] for name in right})
    want = ref.eval_text(ej, jt_, {**TYPES, **{nm: _dt(ty) for nm, ty in rcols}})
    got = sorted(zip(inner.column(0).to_pylist(), inner.column(1).to_pylist(), [repr(v) for v in inner.column(2).to_pylist()]))
    assert got == sorted(zip(jt_["k"], jt_["k_r"], [repr(v) for v in want])) and len(pairs) > 100


@pytest.mark.gpu
def test_group_by_order_by_and_count_distinct_over_a_text_case(gpu):
    from flock_amd.stages import StagedRun, build_query_dag
    n = 3 * FLAG_TILE + 5
    t = shared_table(n)
    key = case([(mod("i", 7, 0), c("u")), (binary(c("i"), "Lt", lit("Int32", 100)), lit_utf8("low")), (binary(c("i"), "Lt", lit("Int32", 300)), lit_utf8(""))])
    labels = ref.eval_text(key, t, TYPES)
    want = {}
    for lab, i in zip(labels, t["i"]):
        cnt, sm = want.get(lab, (0, None))
        want[lab] = (cnt + 1, sm if i is None else i + (sm or 0))
    want = sorted(((k, v[0], v[1], 0 if k is None else v[0]) for k, v in want.items()), key=repr)
    assert None in labels and "" in labels and len(want) > 20
    rb = run(gpu, _group_by_text(key), [(t, COLS)])
    rows = lambda b: list(zip(*[b.column(j).to_pylist() for j in range(b.num_columns)]))
    assert sorted(rows(rb), key=repr) == want
    # the staged run equals the whole plan
    staged = StagedRun(gpu, build_query_dag(_group_by_text(key, parts=4)), instances=1, on_device=True)
    try:
        out = staged.run({"events": batches(t, n)[0]})
    finally:
        staged.close()
    out = out if isinstance(out, list) else [out]
    assert sorted([r for b in out for r in rows(b)], key=repr) == want
    # ORDER BY the label, then k: ascending and descending, NULL labels last
    for desc in (False, True):
        rb = run(gpu, projection([(c("k"), "k")], sort_(scan(), [(key, desc), (c("k"), False)])), [(t, COLS)])
        some = sorted((j for j in range(n) if labels[j] is not None), key=lambda j: (labels[j].encode(), j))
        if desc:
            some = sorted((j for j in range(n) if labels[j] is not None), key=lambda j: ([-b for b in labels[j].encode()] + [1], j))
        assert rb.column(0).to_pylist() == some + [j for j in range(n) if labels[j] is None], desc
    # COUNT(DISTINCT label), COUNT(*)
    rb = run(gpu, _count_distinct(key), [(t, COLS)])
    assert rows(rb) == [(len({v for v in labels if v is not None}), n)]


@pytest.mark.gpu
def test_execute_twice_and_again_with_other_data(gpu):
    from flock_amd.runtime import ExecutionContext
    e = mixed_case()
    ctx = ExecutionContext([projection([(c("k"), "k"), (e, "x"), (lit_utf8("bid"), "kind")])], gpu=gpu)
    try:
        for n in (FLAG_TILE + 1, FLAG_TILE + 1, 3 * TILE + 7, 1):
            t = shared_table(n)
            ctx.feed_data_sources([[batches(t, 3_000)]])
            want = pa.array(ref.eval_text(e, t, TYPES), pa.string())
            for _ in range(2):
                rb = ctx.execute()[0][0]
                assert rb.num_rows == n and rb.column(1).equals(want) and rb.column(2).to_pylist() == ["bid"] * n
            ctx.clean_data_sources()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_text_inside_a_condition_is_refused_at_execute(gpu):
    from flock_amd import FlockGpuError, _ffi
    t = shared_table(1)
    for e, ty, words in ((case([(binary(c("s"), "Eq", lit_utf8("or")), lit("Int32", 1))], lit("Int32", 0)), "Int32", "without one numeric type"),
                         (case([(binary(c("s"), "Eq", lit_utf8("or")), lit_utf8("yes"))], lit_utf8("no")), "Utf8", "without one numeric type")):
        with pytest.raises(FlockGpuError) as err:
            run(gpu, projection([(e, "x")], out_types={"x": ty}), [(t, COLS)])
        assert err.value.code == _ffi.ERR_UNSUPPORTED and words in str(err.value), str(err.value)


BID = [("auction", "Int32"), ("bidder", "Int32"), ("price", "Int32"), ("b_date_time", "ts")]


@pytest.mark.gpu
def test_q14_end_to_end(gpu):
    """NEXMark q14 without its UDF over 100 000 bids whose hours lie on both sides of every boundary (6|7, 7|8, 18|19, 19|20); the three labels all occur."""
    n = 100_000
    r = np.random.default_rng(14)
    day = 1_436_918_400_000
    hours = r.integers(0, 24, n)
    edge = np.array([6, 7, 8, 18, 19, 20])
    hours[::5] = edge[np.arange(len(hours[::5])) % 6]
    within = r.integers(0, 3_600_000, n)
    within[::10] = np.where(np.arange(len(within[::10])) % 2 == 0, 0, 3_599_999)          # the first and the last millisecond of the hour
    ts = (day + r.integers(0, 30, n) * 86_400_000 + hours * 3_600_000 + within).tolist()
    bid = {"auction": r.integers(1000, 2000, n).astype(np.int32).tolist(), "bidder": r.integers(0, 300, n).astype(np.int32).tolist(),
           "price": r.integers(1, 100_000_000, n).astype(np.int32).tolist(), "b_date_time": ts}
    rb = run(gpu, open(os.path.join(PLANS, "q14_bid_time_type.json")).read(), [(bid, BID)], chunk=30_000)
    assert rb.schema.names == ["auction", "bidder", "price", "bid_time_type", "b_date_time"]
    want = []
    for a, b, p, when in zip(bid["auction"], bid["bidder"], bid["price"], ts):
        price = 0.908 * float(p)
        if not (price > 1000000.0 and price < 50000000.0):
            continue
        h = (when // 3_600_000) % 24
        want.append((a, b, price, "dayTime" if 8 <= h <= 18 else "nightTime" if (h <= 6 or h >= 20) else "otherTime", when))
    got = list(zip(rb.column(0).to_pylist(), rb.column(1).to_pylist(), rb.column(2).to_pylist(), rb.column(3).to_pylist(), rb.column(4).cast(pa.int64()).to_pylist()))
    assert got == want and len(want) > 30_000
    assert {w[3] for w in want} == {"dayTime", "nightTime", "otherTime"}
    by_hour = {(w[4] // 3_600_000) % 24: w[3] for w in want}
    assert [by_hour[h] for h in (6, 7, 8, 18, 19, 20)] == ["nightTime", "otherTime", "dayTime", "dayTime", "otherTime", "nightTime"]
