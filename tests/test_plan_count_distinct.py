"""COUNT(DISTINCT x) as an aggregate of HashAggregateExec, grouped and ungrouped (flock_amd/csrc/distinct.hpp A-D1..A-D7): the `distinct_count` entry beside
the ordinary aggregates, every key shape GROUP BY takes, Final / FinalPartitioned over the Partial of the same plan as one pass -- against the plain-Python
sets of tests/count_distinct_ref.py, which a CPU test holds to pyarrow's count_distinct."""
import json
import os

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import count_distinct_ref as ref
from count_distinct_ref import agg_name, dc_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")

TS = {"Timestamp": ["Millisecond", None]}
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string(), "ts": pa.timestamp("ms")}
# keys: kd dense Int32, kw Int64 scattered over 2^40, ks Utf8, kn Int32 with NULL keys; arguments: i l u t s (f: refused)
COLS = [("kd", "Int32"), ("kw", "Int64"), ("ks", "Utf8"), ("kn", "Int32"), ("i", "Int32"), ("l", "Int64"), ("u", "UInt64"), ("t", "ts"), ("s", "Utf8"), ("f", "Float64")]
TYPES = dict(COLS)
TILE = 8192
SIZES = [0, 1, 63, 65, TILE - 1, TILE, TILE + 1, 5 * TILE + 4099]
RESULT = {"dc": lambda t: "UInt64", "count": lambda t: "UInt64", "avg": lambda t: "Float64", "sum": lambda t: "UInt64" if t == "UInt64" else "Int64", "min": lambda t: t,
          "max": lambda t: t}


# ------------------------------------------------------------------ plans
def _dt(t):
    return TS if t == "ts" else t


def _field(name, t, nullable=True):
    return {"data_type": _dt(t), "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


def _c(name, cols=COLS):
    return {"physical_expr": "column", "name": name, "index": [n for n, _ in cols].index(name)}


def _lit(ty, v):
    return {"physical_expr": "literal", "value": {ty: v}}


def _bin(l, op, r):
    return {"physical_expr": "binary_expr", "left": l, "op": op, "right": r}


def _scan(cols=COLS):
    return {"execution_plan": "memory_exec", "schema": {"fields": [_field(n, t) for n, t in cols], "metadata": {}}, "projection": list(range(len(cols)))}


def _filter(inp, pred):
    return {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096, "input": {"execution_plan": "filter_exec", "predicate": pred, "input": inp}}


def _entry(fn, arg, cols=COLS, tag="distinct_count", how="exprs", expr=None, name=None, ty=None):
    at = dict(cols)[arg] if arg else None
    e = expr if expr is not None else (_c(arg, cols) if arg else _lit("UInt8", 1))
    if fn != "dc":
        return {"aggregate_expr": fn, "name": name or agg_name(fn, arg), "data_type": _dt(ty or RESULT[fn](at)), "nullable": True, "expr": e}
    out = {"aggregate_expr": tag, "name": name or dc_name(arg), "data_type": "UInt64", "nullable": True}
    if how == "exprs":    # DistinctCount { name, data_type, state_data_types, exprs, input_data_types }
        out.update({"exprs": [e], "state_data_types": [_dt(at or "Int64")], "input_data_types": [_dt(at or "Int64")]})
    else:
        out["expr"] = e
    return out


def _list_field(name, t):
    item = {"data_type": _dt(t), "dict_id": 0, "dict_is_ordered": False, "name": "item", "nullable": True}
    return {"data_type": {"List": item}, "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": False}


def _state_fields(aggs, cols):
    out = []
    for fn, arg in aggs:
        name, at = agg_name(fn, arg), dict(cols)[arg] if arg else None
        if fn == "dc":
            out.append(_list_field(name + "[count distinct]", at))
        elif fn == "avg":
            out += [_field(name + "[count]", "UInt64"), _field(name + "[sum]", "Float64")]
        else:
            out.append(_field("%s[%s]" % (name, fn), RESULT[fn](at)))
    return out


def agg_node(mode, keys, aggs, inp, cols=COLS, entries=None, group=None):
    """One hash_aggregate_exec.  Partial: the group keys are the input's columns; Final: the Partial's, by position."""
    entries = entries if entries is not None else [_entry(fn, arg, cols) for fn, arg in aggs]
    if group is None:
        group = [[_c(k, cols) if mode == "Partial" else {"physical_expr": "column", "name": k, "index": i}, k] for i, k in enumerate(keys)]
    kf = [_field(k, dict(cols)[k]) for k in keys]
    if aggs is None:
        fields = []
    elif mode == "Partial":
        fields = kf + _state_fields(aggs, cols)
    else:
        fields = kf + [_field(agg_name(fn, arg), RESULT[fn](dict(cols)[arg] if arg else None)) for fn, arg in aggs]
    return {"execution_plan": "hash_aggregate_exec", "mode": mode, "group_expr": group, "aggr_expr": entries, "input": inp,
            "input_schema": {"fields": [_field(n, t) for n, t in cols], "metadata": {}}, "schema": {"fields": fields, "metadata": {}}}


def whole_plan(keys, aggs, inp=None, cols=COLS, mode=None, entries=None, group=None, parts=4):
    """Partial -> [Hash repartition on the keys ->] Final*, as the planner writes SELECT <keys>, <aggs> FROM ... GROUP BY <keys>"""
    partial = agg_node("Partial", keys, aggs, inp or _scan(cols), cols, entries, group)
    if keys:
        mid = {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096,
               "input": {"execution_plan": "repartition_exec", "input": partial,
                         "partitioning": {"Hash": [[{"physical_expr": "column", "name": k, "index": i} for i, k in enumerate(keys)], parts]}}}
    else:
        mid = {"execution_plan": "coalesce_partitions_exec", "input": partial}
    fgroup = None if group is None else [[{"physical_expr": "column", "name": g[1], "index": i}, g[1]] for i, g in enumerate(group)]
    return agg_node(mode or ("FinalPartitioned" if keys else "Final"), keys, aggs, mid, cols, entries, fgroup)


# ------------------------------------------------------------------ tables: {column: [values, None = NULL]}
def make_table(n, seed, null_p=0.0, card="hot", groups=37):
    """card: "one" every row one value; "own" every row its own value (the fullest table); "hot" one value on half the rows over about 100 others.
    The UInt64 column sits at and above 2^63; Int64 values come in pairs v, v + 2^32; the Utf8 argument holds '' and, with null_p, NULL together."""
    r = np.random.default_rng(seed)
    if card == "one":
        base = np.zeros(n, np.int64)
    elif card == "own":
        base = r.permutation(n).astype(np.int64)
    else:
        base = np.where(r.random(n) < 0.5, 0, r.integers(1, 101, n)).astype(np.int64)
    t = {}
    t["kd"] = r.integers(0, groups, n).astype(np.int64).tolist()
    t["kw"] = ((r.integers(0, groups, n).astype(np.int64) * 0x9E3779B1) % (1 << 40) - (1 << 39)).tolist()
    t["ks"] = ["key-%d" % k if k else "" for k in r.integers(0, groups, n).tolist()]
    t["kn"] = [None if k == 0 else k for k in r.integers(0, groups, n).tolist()]
    t["i"] = (base * 7 - 300).tolist()
    t["l"] = (base // 2 * 10**10 + (base % 2) * 2**32).tolist()
    t["u"] = [2**63 + int(b) * 4097 for b in base.tolist()]
    t["t"] = (1_436_918_400_000 + base * 1000).tolist()
    t["s"] = ["" if b == 1 else "v%d" % b for b in base.tolist()]
    t["f"] = [float(b) for b in base.tolist()]
    if null_p > 0:
        for c in ("i", "l", "u", "t", "s"):
            ok = np.zeros(n, bool) if null_p >= 1 else r.random(n) >= null_p
            t[c] = [v if o else None for v, o in zip(t[c], ok.tolist())]
    return t


def record_batch(t, lo=0, hi=None, cols=COLS):
    arrs = []
    for name, ty in cols:
        v = t[name][lo:hi]
        arrs.append(pa.array(v, pa.int64()).cast(_PA[ty]) if ty == "ts" else pa.array(v, _PA[ty]))
    return pa.record_batch(arrs, names=[c for c, _ in cols])


def batches(t, k=1, cols=COLS):
    n = len(t[cols[0][0]])
    cuts = [n * j // k for j in range(k + 1)]
    return [record_batch(t, a, b, cols) for a, b in zip(cuts[:-1], cuts[1:])]


def out_rows(out):
    rows = []
    for rb in out:
        cs = [(c.cast(pa.int64()) if pa.types.is_timestamp(c.type) else c).to_pylist() for c in rb.columns]
        rows += list(zip(*cs)) if cs else []
    return rows


@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def run(gpu, plan, feeds, ctx=None):
    """feeds: per leaf, a list of batches -> the output batches"""
    from flock_amd.runtime import ExecutionContext, collect
    own = ctx is None
    ctx = ctx or ExecutionContext([plan], gpu=gpu)
    try:
        return collect(ctx, [[f] for f in feeds])[0]
    finally:
        if own:
            ctx.close()


def check(gpu, t, keys, aggs, k=1, cols=COLS, **kw):
    out = run(gpu, whole_plan(keys, aggs, cols=cols, **kw), [batches(t, k, cols)])
    want = ref.sort_rows(ref.aggregate(t, keys, aggs), len(keys))
    got = ref.sort_rows(out_rows(out), len(keys))
    assert got == want, (keys, aggs, len(got), len(want), [p for p in zip(got, want) if p[0] != p[1]][:3])
    for rb in out:
        assert rb.schema.names == list(keys) + [agg_name(fn, arg) for fn, arg in aggs]
        assert [f.type for f in rb.schema][len(keys):] == [_PA[RESULT[fn](dict(cols)[arg] if arg else None)] for fn, arg in aggs]
    if not keys:
        assert len(got) == 1      # A-D3: no GROUP BY -> exactly one row, over no rows too
    return got


# ------------------------------------------------------------------ CPU: the reference
def test_reference_on_hand_worked_rows():
    t = {"g": [1, 1, 2, 2, None, None, 3], "v": [5, 5, None, 7, 8, 8, None]}
    assert ref.sort_rows(ref.aggregate(t, ["g"], [("dc", "v")]), 1) == [(None, 1), (1, 1), (2, 1), (3, 0)]
    assert ref.aggregate(t, [], [("dc", "v"), ("count", None), ("count", "v"), ("dc", "g")]) == [(3, 7, 5, 3)]
    assert ref.aggregate({"v": []}, [], [("dc", "v"), ("count", None)]) == [(0, 0)]          # no rows: one row, 0
    assert ref.aggregate({"g": [], "v": []}, ["g"], [("dc", "v")]) == []
    assert ref.aggregate({"s": ["", None, "", "a"]}, [], [("dc", "s")]) == [(2,)]             # '' is a value, not NULL
    assert ref.aggregate({"v": [7, 7 + 2**32]}, [], [("dc", "v")]) == [(2,)]


@pytest.mark.parametrize("seed", [1, 2])
def test_reference_against_pyarrow(seed):
    t = make_table(3000, seed, 0.3)
    tab = pa.Table.from_batches([record_batch(t)])
    for arg in ("i", "l", "u", "s"):
        assert ref.aggregate(t, [], [("dc", arg)]) == [(pc.count_distinct(tab.column(arg)).as_py(),)]
        for keys in (["kd"], ["kn"], ["ks"], ["kd", "ks"]):
            got = tab.group_by(keys, use_threads=False).aggregate([(arg, "count_distinct")])
            rows = list(zip(*[got.column(k).to_pylist() for k in keys], got.column(arg + "_count_distinct").to_pylist()))
            assert ref.sort_rows(rows, len(keys)) == ref.sort_rows(ref.aggregate(t, keys, [("dc", arg)]), len(keys)), (arg, keys)
    hand = pa.table({"g": pa.array([1, 1, 2, 2, None, None, 3], pa.int32()), "v": pa.array([5, 5, None, 7, 8, 8, None], pa.int32())})
    got = hand.group_by(["g"], use_threads=False).aggregate([("v", "count_distinct")])
    assert sorted(zip(got.column("g").to_pylist(), got.column("v_count_distinct").to_pylist()), key=lambda r: (r[0] is not None, r[0])) == [(None, 1), (1, 1), (2, 1), (3, 0)]


# ------------------------------------------------------------------ CPU: parsing, explain, refusals
def test_both_tags_and_both_argument_forms_parse():
    from flock_amd.runtime import explain
    for tag in ("distinct_count", "count_distinct"):
        for how in ("exprs", "expr"):
            entries = [_entry("count", None), _entry("dc", "i", tag=tag, how=how), _entry("dc", "s", tag=tag, how=how), _entry("max", "t")]
            aggs = [("count", None), ("dc", "i"), ("dc", "s"), ("max", "t")]
            for keys in ([], ["kd"], ["kd", "ks"]):
                text = explain(whole_plan(keys, aggs, entries=entries))
                first = text.splitlines()[0]
                assert first.startswith("Aggregate(%s, single pass) [" % ("FinalPartitioned" if keys else "Final")), text
                for col in ["COUNT(UInt8(1)):UInt64", "COUNT(DISTINCT i):UInt64", "COUNT(DISTINCT s):UInt64", "MAX(t):Timestamp(ms)"] + ["%s:%s" % (k, TYPES[k]) for k in keys]:
                    assert col in first, (col, text)
                assert "Aggregate(Partial)" not in text and "Repartition" not in text, text     # one aggregation over the Partial's input
                assert text.splitlines()[1].strip().startswith("Scan"), text


def test_a_computed_argument_goes_through_a_projection():
    from flock_amd.runtime import explain
    case = {"physical_expr": "case_expr", "expr": None, "when_then_expr": [[_bin(_c("i"), "Lt", _lit("Int32", 100)), _c("l")]], "else_expr": None}
    entries = [_entry("dc", None, expr=case, name="COUNT(DISTINCT CASE)"), _entry("count", None)]
    text = explain(whole_plan(["kd"], None, entries=entries))
    assert "COUNT(DISTINCT CASE):UInt64" in text.splitlines()[0] and text.splitlines()[1].strip().startswith("Project"), text


def test_the_fixture_parses():
    from flock_amd.runtime import explain
    text = explain(open(os.path.join(PLANS, "q15_bid_stats.json")).read())
    first = text.splitlines()[0]
    assert first.startswith("Aggregate(FinalPartitioned, single pass) [day:Timestamp(ms), "), text
    for col in ("total_bids:UInt64", "bidders:UInt64", "auctions:UInt64", "rank1_bidders:UInt64"):
        assert col in first, text
    assert "date_trunc('day', b_date_time)" in text, text


def _refused(plan, *words):
    from flock_amd import FlockGpuError
    from flock_amd.runtime import explain
    with pytest.raises(FlockGpuError) as e:
        explain(plan)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals_name_their_cause():
    _refused(whole_plan(["kd"], [("dc", "f")]), "distinct_count needs an integer or Utf8 column")
    _refused(whole_plan([], [("dc", "f")]), "distinct_count needs an integer or Utf8 column")
    fl = _bin({"physical_expr": "cast_expr", "expr": _c("i"), "cast_type": "Float64"}, "Multiply", _lit("Float64", 0.5))
    _refused(whole_plan(["kd"], None, entries=[_entry("dc", None, expr=fl, name="x")]), "distinct_count needs an integer or Utf8 column")
    two = _entry("dc", "i")
    two["exprs"] = [_c("i"), _c("l")]
    _refused(whole_plan(["kd"], None, entries=[two]), "distinct_count over 2 argument expressions")
    five = [("dc", c) for c in ("i", "l", "u", "t", "s")]
    _refused(whole_plan(["kd"], five), "more than 4 distinct counts")
    _refused(whole_plan([], five), "more than 4 distinct counts")
    # the accumulator limit of the ordinary aggregates is unchanged beside a distinct count (A-D4)
    _refused(whole_plan([], [("dc", "i")] + [(fn, c) for c in "il" for fn in ("count", "sum", "min", "max")] + [("count", None)]), "more than 8 accumulators")
    # an unknown function is refused in the words of today; the list may name the new function
    _refused(whole_plan(["kd"], None, entries=[dict(_entry("count", "i"), aggregate_expr="approx_distinct")]), "aggregate function 'approx_distinct' (supported: count, max, min, sum, avg")


def test_a_partial_that_anything_else_consumes_is_refused():
    aggs = [("count", None), ("dc", "i")]
    partial = agg_node("Partial", ["kd"], aggs, _scan())
    _refused(partial, "distinct_count", "list state")                                    # at the plan root: what a stage cut leaves
    rep = {"execution_plan": "repartition_exec", "input": partial, "partitioning": {"Hash": [[{"physical_expr": "column", "name": "kd", "index": 0}], 4]}}
    _refused(rep, "distinct_count", "list state")
    _refused({"execution_plan": "global_limit_exec", "input": partial, "limit": 3}, "distinct_count", "list state")   # feeding another operator
    # a Final whose lists are not the Partial's does not swallow it
    other = agg_node("FinalPartitioned", ["kd"], [("count", None), ("dc", "l")], rep)
    _refused(other, "distinct_count", "list state")
    # the stage splitter is unchanged: the stage it cuts at the hash repartition ends in that Partial
    from flock_amd.stages import build_query_dag
    stages = build_query_dag(whole_plan(["kd"], aggs))
    assert len(stages) == 2
    _refused(stages[0].plan, "distinct_count", "list state")


def test_a_final_over_a_scan_fails_on_the_list_field():
    state = {"execution_plan": "memory_exec", "projection": [0, 1, 2],
             "schema": {"fields": [_field("kd", "Int32"), _field("COUNT(UInt8(1))[count]", "UInt64"), _list_field("COUNT(DISTINCT i)[count distinct]", "Int32")], "metadata": {}}}
    _refused(agg_node("FinalPartitioned", ["kd"], [("count", None), ("dc", "i")], state), "column 'COUNT(DISTINCT i)[count distinct]': data type outside {Int32, Int64, UInt64, Float64, Utf8, Timestamp(ms)}")


def test_a_window_entry_is_refused():
    for tag in ("distinct_count", "count_distinct"):
        w = {"window_expr": "aggregate_window_expr", "aggregate": _entry("dc", "i", tag=tag, how="expr"), "partition_by": [_c("kd")], "order_by": [], "window_frame": None}
        plan = {"execution_plan": "window_agg_exec", "input": _scan(), "window_expr": [w], "input_schema": {"fields": [], "metadata": {}}, "schema": {"fields": [], "metadata": {}}}
        _refused(plan, "window function '%s' (supported: ROW_NUMBER, COUNT, SUM, MIN, MAX, AVG)" % tag)


# explain's text for two plans without a distinct count, recorded from the commit before this feature
GOLDEN_AGGREGATE = ("Project [MAX(c1):Int64, MIN(c2):Float64, c3:Utf8]\n  Aggregate(FinalPartitioned) [c3:Utf8, MAX(c1):Int64, MIN(c2):Float64]  <- generic (relops.hip)\n"
                    "    Repartition(Hash, 8) [c3:Utf8, MAX(c1)[max]:Int64, MIN(c2)[min]:Float64]\n      Aggregate(Partial) [c3:Utf8, MAX(c1)[max]:Int64, MIN(c2)[min]:Float64]  <- generic (relops.hip)\n"
                    "        Filter [c1:Int64, c2:Float64, c3:Utf8]  <- generic (relops.hip)\n          Scan() [c1:Int64, c2:Float64, c3:Utf8]\n")
Q5 = "Project [auction:Int32, num:UInt64]\n  Join [auction:Int32, num:UInt64, maxn:UInt64]  <- fused q5 count / max / select (q5.hip)\n"


def test_a_node_without_a_distinct_count_explains_exactly_as_before():
    from flock_amd.runtime import explain
    assert explain(open(os.path.join(PLANS, "golden_aggregate.json")).read()) == GOLDEN_AGGREGATE
    assert explain(open(os.path.join(PLANS, "q5.json")).read()) == Q5
    # ... and beside the new tests' own plans: the same lists without the distinct count keep their two stages
    text = explain(whole_plan(["kd"], [("count", None), ("max", "t")]))
    assert "single pass" not in text and "Aggregate(Partial)" in text and "Repartition(Hash, 4)" in text, text


# ------------------------------------------------------------------ GPU 1: row counts x NULL rates x argument types
_tables = {}


def table(n, null_p, card="hot"):
    """One table per (rows, NULL rate, cardinality): built once, shared, never changed."""
    key = (n, null_p, card)
    if key not in _tables:
        _tables[key] = make_table(n, 1000 + n % 977 + int(null_p * 10) + len(card), null_p, card)
    return _tables[key]


@pytest.mark.gpu
@pytest.mark.parametrize("null_p", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("n", SIZES)
def test_every_argument_type_grouped_and_ungrouped(gpu, n, null_p):
    t = table(n, null_p)
    for keys in ([], ["kd"]):
        check(gpu, t, keys, [("dc", "i"), ("dc", "l"), ("dc", "u"), ("dc", "t")])
        got = check(gpu, t, keys, [("dc", "s"), ("count", None)])
        if null_p >= 1:
            assert all(r[len(keys)] == 0 for r in got)       # nothing but NULLs: 0, never NULL


# ------------------------------------------------------------------ GPU 2: cardinality x key shape
KEYS = {"none": [], "dense_i32": ["kd"], "scattered_i64": ["kw"], "utf8": ["ks"], "null_keys": ["kn"], "i32_utf8": ["kd", "ks"]}


@pytest.mark.gpu
@pytest.mark.parametrize("card", ["one", "own", "hot"])
@pytest.mark.parametrize("shape", sorted(KEYS))
def test_every_key_shape_and_cardinality(gpu, shape, card):
    t = table(TILE + 1, 0.3 if card == "hot" else 0.0, card)
    got = check(gpu, t, KEYS[shape], [("count", None), ("dc", "i"), ("dc", "l"), ("dc", "s")])
    if shape == "null_keys":
        assert got[0][0] is None      # NULL keys form one group


@pytest.mark.gpu
def test_adversarial_values(gpu):
    v = 123_456_789
    t = {c: [0] * 8 for c, _ in COLS}
    t["ks"], t["s"], t["f"] = [""] * 8, [None] * 8, [0.0] * 8
    t["kd"] = [1, 1, 1, 2, 2, 3, 3, 1]
    t["l"] = [v, v + 2**32, v, v, v - 2**32, None, None, v + 2**32]          # v and v + 2^32 in one group count as two; v counts once in each group
    t["i"] = [5, 5, None, 5, -5, None, None, 2**31 - 1]
    t["u"] = [2**63, 2**64 - 1, 2**63, 2**63, 1, None, None, 0]
    t["s"] = ["", None, "", "a", "", None, None, "a"]                          # '' and NULL together
    got = check(gpu, t, ["kd"], [("dc", "l"), ("dc", "i"), ("dc", "u"), ("dc", "s")])
    assert got == [(1, 2, 2, 3, 2), (2, 2, 2, 2, 2), (3, 0, 0, 0, 0)]          # group 3: every argument NULL -> 0
    assert check(gpu, t, [], [("dc", "l"), ("dc", "i"), ("dc", "u"), ("dc", "s")]) == [(3, 3, 4, 2)]


# ------------------------------------------------------------------ GPU 3: beside other aggregates, batching, modes
# two distinct counts over different columns next to COUNT(*), MAX and AVG: the four accumulators a GROUP BY takes (AVG takes two), unchanged (A-D4)
MIXED = [("count", None), ("dc", "i"), ("max", "t"), ("dc", "s"), ("avg", "i")]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["none", "dense_i32", "i32_utf8"])
def test_beside_other_aggregates_in_the_plans_order(gpu, shape):
    t = table(2 * TILE + 77, 0.3)
    keys = KEYS[shape]
    check(gpu, t, keys, MIXED if keys else MIXED + [("count", "l"), ("min", "l"), ("sum", "i")])      # (no GROUP BY: eight accumulators)
    check(gpu, t, keys, [("dc", "l"), ("count", None)])            # the distinct count first
    check(gpu, t, keys, [("dc", "u")])                             # ... and alone


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["none", "dense_i32"])
def test_batches_and_repeats_change_nothing(gpu, shape):
    """One batch and three give identical results; a second execute finds the first one's table size (sized from the pairs it saw) -- and a third, over a
    relation with many more distinct values than that, overflows it and is repeated over a table that holds."""
    from flock_amd.runtime import ExecutionContext
    keys = KEYS[shape]
    aggs = [("dc", "i"), ("count", None), ("dc", "s")]
    few, many = table(5 * TILE + 4099, 0.3), table(5 * TILE + 4099, 0.0, "own")
    want = {id(x): ref.sort_rows(ref.aggregate(x, keys, aggs), len(keys)) for x in (few, many)}
    ctx = ExecutionContext([whole_plan(keys, aggs)], gpu=gpu)
    try:
        for x, k in ((few, 1), (few, 3), (many, 3), (few, 1)):
            assert ref.sort_rows(out_rows(run(gpu, None, [batches(x, k)], ctx)), len(keys)) == want[id(x)]
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["Final", "FinalPartitioned"])
def test_final_modes_over_a_hash_repartition(gpu, mode):
    t = table(TILE + 1, 0.3)
    check(gpu, t, ["kd"], MIXED, k=2, mode=mode, parts=8)
    check(gpu, t, ["kn", "ks"], [("dc", "l"), ("count", None)], k=2, mode=mode, parts=3)


# ------------------------------------------------------------------ GPU 4: position in the plan
@pytest.mark.gpu
def test_above_a_filter(gpu):
    t = table(2 * TILE + 77, 0.3)
    pred = _bin(_bin(_c("kd"), "Modulo", _lit("Int32", 3)), "Eq", _lit("Int32", 1))
    kept = {c: [v for v, k in zip(vals, t["kd"]) if k % 3 == 1] for c, vals in t.items()}
    aggs = [("count", None), ("dc", "i"), ("dc", "s"), ("max", "l")]
    for keys in ([], ["kd"]):
        out = run(gpu, whole_plan(keys, aggs, _filter(_scan(), pred)), [batches(t, 2)])
        assert ref.sort_rows(out_rows(out), len(keys)) == ref.sort_rows(ref.aggregate(kept, keys, aggs), len(keys))


@pytest.mark.gpu
def test_below_a_sort_and_limit(gpu):
    t = table(2 * TILE + 77, 0.3)
    aggs = [("dc", "i"), ("count", None)]
    ocols = [("kd", "Int32"), (dc_name("i"), "UInt64"), ("COUNT(UInt8(1))", "UInt64")]
    sort = {"execution_plan": "sort_exec", "input": whole_plan(["kd"], aggs), "expr": [{"expr": _c("kd", ocols), "options": {"descending": True, "nulls_first": False}}]}
    out = run(gpu, {"execution_plan": "global_limit_exec", "input": sort, "limit": 5}, [batches(t)])
    assert out_rows(out) == sorted(ref.aggregate(t, ["kd"], aggs), reverse=True)[:5]


@pytest.mark.gpu
def test_as_a_join_input(gpu):
    t = table(2 * TILE + 77, 0.3)
    aggs = [("dc", "s"), ("dc", "l")]
    lcols = [("want", "Int32")]
    ocols = [("kd", "Int32"), (dc_name("s"), "UInt64"), (dc_name("l"), "UInt64")]
    left = {"execution_plan": "memory_exec", "schema": {"fields": [_field("want", "Int32")], "metadata": {}}, "projection": [0]}
    join = {"execution_plan": "hash_join_exec", "left": left, "right": whole_plan(["kd"], aggs), "join_type": "Inner", "mode": "CollectLeft",
            "on": [[_c("want", lcols), _c("kd", ocols)]], "schema": {"fields": [_field(n, ty) for n, ty in lcols + ocols], "metadata": {}}}
    wanted = [3, 5, 5, 1000, 0]
    out = run(gpu, join, [[pa.record_batch([pa.array(wanted, pa.int32())], names=["want"])], batches(t)])
    by_key = {r[0]: r for r in ref.aggregate(t, ["kd"], aggs)}
    assert sorted(out_rows(out)) == sorted((w,) + by_key[w] for w in wanted if w in by_key)


# ------------------------------------------------------------------ GPU 5: the fixture
@pytest.mark.gpu
def test_q15_bid_stats_over_generated_bids(gpu):
    """COUNT(*), COUNT(DISTINCT bidder), COUNT(DISTINCT auction), COUNT(DISTINCT CASE WHEN price < 10000 THEN bidder END) GROUP BY date_trunc('day', b_date_time)
    over a few thousand bids under NEXMark's skew (half of them on one auction, three quarters from one bidder), timestamps tied and spread over four days."""
    plan = json.load(open(os.path.join(PLANS, "q15_bid_stats.json")))
    r = np.random.default_rng(15)
    n = 6000
    day = 86_400_000
    auction = np.where(r.random(n) < 0.5, 1007, r.integers(1000, 1200, n)).astype(np.int32)
    bidder = np.where(r.random(n) < 0.75, 42, r.integers(0, 300, n)).astype(np.int32)
    price = r.integers(100, 20_000, n).astype(np.int32)
    ts = 1_436_918_400_000 - 5_000 + (np.sort(r.integers(0, 4 * day, n)) // 60_000) * 60_000       # ties: whole minutes; the first day starts before midnight
    rb = pa.record_batch([pa.array(auction), pa.array(bidder), pa.array(price), pa.array(ts, pa.int64()).cast(pa.timestamp("ms"))],
                         names=["auction", "bidder", "price", "b_date_time"])
    t = {"day": (ts // day * day).tolist(), "bidder": bidder.tolist(), "auction": auction.tolist(),
         "cheap": [b if p < 10000 else None for b, p in zip(bidder.tolist(), price.tolist())]}
    want = ref.sort_rows(ref.aggregate(t, ["day"], [("count", None), ("dc", "bidder"), ("dc", "auction"), ("dc", "cheap")]), 1)
    assert len(want) == 5
    for k in (1, 3):
        cuts = [n * j // k for j in range(k + 1)]
        out = run(gpu, plan, [[rb.slice(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]])
        assert ref.sort_rows(out_rows(out), 1) == want
        assert out[0].schema.names == ["day", "total_bids", "bidders", "auctions", "rank1_bidders"]
