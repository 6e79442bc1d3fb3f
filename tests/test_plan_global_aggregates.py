"""Aggregates without GROUP BY (reduce.hpp): COUNT / SUM / MIN / MAX / AVG, any list of them, in Partial and Final mode, over a scan, a filter (read
under its flag words), and above / below the other operators -- against oracle/generic_ops.py hash_aggregate_exec with group_by=[] (tests/global_agg_ref.py)."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from global_agg_ref import agg_name, partial_state, reference_is_exact, reference_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")

_TS = {"Timestamp": ["Millisecond", None]}
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string(), "ts": pa.timestamp("ms")}
COLS = [("i", "Int32"), ("l", "Int64"), ("u", "UInt64"), ("t", "ts"), ("f", "Float64"), ("p", "Int32"), ("s", "Utf8")]
NUMERIC = COLS[:6]
TYPES = dict(COLS)
TILE = 8192                       # rows of one flag tile
SIZES = [0, 1, 63, 65, TILE - 1, TILE, TILE + 1, 5 * TILE + 4099]
# the range a SUM's result type holds (the reference adds Python integers: it must stay inside, GROUP BY's wrap is not under test)
SUM_RANGE = {"i": (-2**63, 2**63 - 1), "l": (-2**63, 2**63 - 1), "p": (-2**63, 2**63 - 1), "u": (0, 2**64 - 1), "t": (-2**63, 2**63 - 1)}
RESULT = {"count": lambda t: "UInt64", "avg": lambda t: "Float64", "sum": lambda t: "UInt64" if t == "UInt64" else "Int64", "min": lambda t: t, "max": lambda t: t}
SIX = lambda v: [("count", None), ("count", v), ("sum", v), ("min", v), ("max", v), ("avg", v)]


# ------------------------------------------------------------------ plans
def _dt(t):
    return _TS if t == "ts" else t


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


def _entry(fn, arg, cols=COLS, expr=None, ty=None):
    ty = ty or RESULT[fn](dict(cols)[arg] if arg else None)
    return {"aggregate_expr": fn, "name": agg_name(fn, arg), "data_type": _dt(ty), "nullable": True,
            "expr": expr if expr is not None else (_c(arg, cols) if arg else _lit("UInt8", 1))}


def state_fields(aggs, cols=COLS):
    out = []
    for fn, arg in aggs:
        name, ty = agg_name(fn, arg), RESULT[fn](dict(cols)[arg] if arg else None)
        if fn == "avg":
            out += [_field(name + "[count]", "UInt64"), _field(name + "[sum]", "Float64")]
        else:
            out.append(_field("%s[%s]" % (name, fn), ty))
    return out


def agg_node(mode, aggs, inp, cols=COLS, entries=None, fields=None):
    """The node's own schema (what the stage split gives the leaf of the consuming stage): the state columns of a Partial, the results of a Final."""
    if fields is None and aggs is not None:
        fields = state_fields(aggs, cols) if mode == "Partial" else [_field(agg_name(fn, arg), RESULT[fn](dict(cols)[arg] if arg else None)) for fn, arg in aggs]
    return {"execution_plan": "hash_aggregate_exec", "mode": mode, "group_expr": [], "aggr_expr": entries or [_entry(fn, arg, cols) for fn, arg in aggs], "input": inp,
            "input_schema": {"fields": [_field(n, t) for n, t in cols], "metadata": {}}, "schema": {"fields": fields or [], "metadata": {}}}


def whole_plan(aggs, inp=None, cols=COLS):
    """Partial -> CoalescePartitions -> Final, as the planner writes SELECT <aggs> FROM ..."""
    return agg_node("Final", aggs, {"execution_plan": "coalesce_partitions_exec", "input": agg_node("Partial", aggs, inp or _scan(cols), cols)}, cols)


# ------------------------------------------------------------------ tables: {name: (values, valid)}
def make_table(n, seed, null_p, cols=NUMERIC):
    """Values under which the reference is exact (checked by reference_is_exact in every test): Int64 / Timestamp around 1e12, UInt64 multiples of 2^12
    with ONE value at or above 2^63 (a SUM of two would leave UInt64), Float64 with both infinities and no NaN / -0.0."""
    r = np.random.default_rng(seed)
    t = {}
    for name, ty in cols:
        if ty == "Int32":
            v = r.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
        elif ty == "Int64":
            v = r.integers(-10**12, 10**12, n, dtype=np.int64)
        elif ty == "ts":
            v = 1_436_918_400_000 + r.integers(0, 10**9, n, dtype=np.int64)
        elif ty == "UInt64":
            v = r.integers(0, 2**20, n, dtype=np.int64).astype(np.uint64) << np.uint64(12)
            if n:
                v[int(r.integers(0, n))] = np.uint64(2**63) + (np.uint64(int(r.integers(0, 2**20))) << np.uint64(12))
        else:
            v = np.round(r.normal(0, 1e6, n), 3)
            v[v == 0] = 1.0
            if n > 2:
                v[int(r.integers(0, n))], v[int(r.integers(0, n))] = np.inf, -np.inf
        ok = np.ones(n, bool) if null_p == 0 else np.zeros(n, bool) if null_p >= 1 else r.random(n) >= null_p
        t[name] = (v, ok)
    return t


def record_batch(t, lo=0, hi=None, cols=NUMERIC):
    arrs = []
    for name, ty in cols:
        v, ok = t[name]
        hi_ = len(v) if hi is None else hi
        if ty == "Utf8":
            arrs.append(pa.array([x if o else None for x, o in zip(v[lo:hi_].tolist(), ok[lo:hi_].tolist())], pa.string()))
        else:
            a = pa.array(v[lo:hi_], mask=~ok[lo:hi_])
            arrs.append(a.cast(_PA[ty]) if ty == "ts" else a)
    return pa.record_batch(arrs, names=[c for c, _ in cols])


def batches(t, k=1, cols=NUMERIC):
    n = len(t[cols[0][0]][0])
    cuts = [n * j // k for j in range(k + 1)]
    return [record_batch(t, a, b, cols) for a, b in zip(cuts[:-1], cuts[1:])]


def out_row(rb):
    assert rb.num_rows == 1, rb.num_rows
    row = []
    for i in range(rb.num_columns):
        c = rb.column(i)
        if pa.types.is_timestamp(c.type):
            c = c.cast(pa.int64())
        row.append(c.to_pylist()[0])
    return row


def out_types(rb):
    return ["ts" if pa.types.is_timestamp(f.type) else {pa.int32(): "Int32", pa.int64(): "Int64", pa.uint64(): "UInt64", pa.float64(): "Float64"}[f.type] for f in rb.schema]


def row_bits(row):
    return tuple(("f", np.float64(x).view(np.uint64).item()) if isinstance(x, float) else x for x in row)


def same_row(got, want):
    """bit-identical: floats by their bits (an AVG is one IEEE division of exact operands), None = NULL"""
    return row_bits(got) == row_bits(want)


@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def run(gpu, plan, feeds):
    """feeds: per leaf, a list of batches"""
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        out = collect(ctx, [[f] for f in feeds])[0]
    finally:
        ctx.close()
    assert len(out) == 1
    return out[0]


# ------------------------------------------------------------------ CPU: the reference
def _hand(rows, names):
    return {name: (np.array([0 if r[k] is None else r[k] for r in rows], np.int64), np.array([r[k] is not None for r in rows], bool)) for k, name in enumerate(names)}


def test_reference_on_hand_worked_rows():
    t = _hand([(4, None), (None, None), (7, None), (-3, None), (None, None)], ["v", "z"])
    assert reference_row(t, SIX("v")) == [5, 3, 8, -3, 7, 8 / 3]
    assert reference_row(t, SIX("z")) == [5, 0, None, None, None, None]                    # an all-NULL column
    assert reference_row(_hand([], ["v"]), SIX("v")) == [0, 0, None, None, None, None]     # no rows: one row all the same
    assert partial_state(t, [("avg", "v"), ("max", "v"), ("count", None)]) == [3, 8.0, 7, 5]
    assert partial_state(_hand([], ["v"]), [("avg", "v"), ("sum", "v")]) == [0, 0.0, None]


@pytest.mark.parametrize("seed", [1, 2])
def test_reference_against_pyarrow(seed):
    t = make_table(3000, seed, 0.3)
    rb = record_batch(t)
    for name, ty in NUMERIC:
        col = rb.column(name).cast(pa.int64()) if ty == "ts" else rb.column(name)
        aggs = [("count", name), ("min", name), ("max", name)] + ([] if ty == "Float64" else [("sum", name), ("avg", name)])
        assert reference_is_exact(t, aggs, SUM_RANGE)
        got = dict(zip([fn for fn, _ in aggs], reference_row(t, aggs)))
        assert got["count"] == pc.count(col).as_py() and got["min"] == pc.min(col).as_py() and got["max"] == pc.max(col).as_py()
        if ty != "Float64":
            exact = sum(int(x) for x in col.to_pylist() if x is not None)
            assert got["sum"] == exact == pc.sum(col).as_py()
            assert got["avg"] == exact / got["count"]


# ------------------------------------------------------------------ CPU: parsing, refusals, NULL dropping, stage split
def test_every_function_and_type_explains():
    from flock_amd.runtime import explain
    aggs = [("count", None)] + [(fn, c) for c, ty in NUMERIC for fn in ("count", "min", "max")] + [(fn, c) for c in "ilu" for fn in ("sum", "avg")]
    for k in range(0, len(aggs), 4):     # (several aggregates in one node, within the accumulator limit)
        part = aggs[k:k + 4]
        text = explain(agg_node("Partial", part, _scan()))
        for f in state_fields(part):
            ty = f["data_type"]
            shown = "Timestamp(ms)" if ty == _TS else ty
            assert "%s:%s" % (f["name"], shown) in text, (f["name"], text)
        text = explain(whole_plan(part))
        for fn, arg in part:
            ty = RESULT[fn](TYPES[arg] if arg else None)
            assert "%s:%s" % (agg_name(fn, arg), "Timestamp(ms)" if ty == "ts" else ty) in text.splitlines()[0], (fn, arg, text)
    # AVG's two state columns, by name and type
    text = explain(agg_node("Partial", [("avg", "l")], _scan()))
    assert "AVG(l)[count]:UInt64" in text and "AVG(l)[sum]:Float64" in text


@pytest.mark.parametrize("aggs,words", [
    ([("sum", "f")], "sum needs an integer column"),
    ([("avg", "f")], "avg needs an integer column"),
    ([("max", "s")], "max needs an integer column"),
    ([("count", "s")], "count needs an integer column"),
    ([("count", None), ("sum", "s")], "sum needs an integer column"),
    ([("avg", "i"), ("avg", "l"), ("avg", "u"), ("avg", "p"), ("count", None)], "more than 8 accumulators"),
    ([(fn, c) for c in "il" for fn in ("count", "sum", "min", "max")] + [("count", None)], "more than 8 accumulators"),
])
def test_refusals_name_their_cause(aggs, words):
    from flock_amd import FlockGpuError
    from flock_amd.runtime import explain
    with pytest.raises(FlockGpuError, match=words):
        explain(agg_node("Partial", aggs, _scan()))


def test_required_columns_and_count_star_alone():
    """`explain` shows what a leaf is read for, not what it may drop: the NULL-dropping rule -- a leaf column may lose its NULL rows only when EVERY
    aggregate of the node takes that column -- is held to at execute (test_null_rows_are_dropped_only_where_every_aggregate_skips_them)."""
    from flock_amd.runtime import explain
    # COUNT(*) alone: nothing of the leaf is read, the plan still explains (the leaf has a row count)
    assert "COUNT(UInt8(1)):UInt64" in explain(whole_plan([("count", None)]))
    for aggs in ([("count", None), ("max", "i")], [("min", "i"), ("max", "i")], [("sum", "i"), ("count", "l")]):
        assert explain(agg_node("Partial", aggs, _scan())).splitlines()[1].strip().startswith("Scan")


def test_lone_max_explains_as_ever_and_recognition_holds():
    from flock_amd import load
    from flock_amd.runtime import explain
    import ctypes as C
    text = explain(whole_plan([("max", "i")]))
    assert text.splitlines()[0].strip().startswith("Aggregate") and "MAX(i):Int32" in text.splitlines()[0]
    lib = load()
    for name, q in (("q5", 5), ("q7", 7)):
        raw = open(os.path.join(PLANS, name + ".json"), "rb").read()
        query = C.c_int(-1)
        assert lib.flockgpu_plan_recognise(raw, len(raw), C.byref(query)) == 0 and query.value == q


def test_stage_split_is_that_of_q7s_max():
    from flock_amd.runtime import explain
    from flock_amd.stages import build_query_dag
    aggs = SIX("l") + [("max", "t")]
    new, old = build_query_dag(whole_plan(aggs)), build_query_dag(whole_plan([("max", "i")]))
    assert len(new) == len(old) == 2

    def shape(o):
        if isinstance(o, dict):
            return {k: shape(v) for k, v in o.items() if k not in ("aggr_expr", "schema")}
        if isinstance(o, list):
            return [shape(x) for x in o]
        return o
    assert [shape(s.plan) for s in new] == [shape(s.plan) for s in old]
    assert [s.inputs for s in new] == [s.inputs for s in old]
    assert new[0].plan["execution_plan"] == "coalesce_partitions_exec" and new[0].plan["input"]["mode"] == "Partial" and new[1].plan["mode"] == "Final"
    for s in new:
        explain(s.plan)


# ------------------------------------------------------------------ GPU 1: every function and type
LISTS = {
    "six_i32": SIX("i"), "six_i64": SIX("l"), "six_u64": SIX("u"),
    "ts_f64": [("min", "t"), ("max", "t"), ("min", "f"), ("max", "f"), ("count", "f")],
    "mixed": [("max", "t"), ("sum", "i"), ("count", None), ("avg", "l"), ("min", "u"), ("count", "p"), ("min", "f")],
}
_refs = {}


def table_and_reference(n, null_p, name):
    """One table per (rows, NULL rate), one reference row per list over it -- computed once, shared, never changed."""
    key = (n, null_p)
    if key not in _refs:
        _refs[key] = (make_table(n, 1000 + n % 977 + int(null_p * 10), null_p), {})
    t, rows = _refs[key]
    if name not in rows:
        assert reference_is_exact(t, LISTS[name], SUM_RANGE), (n, null_p, name)
        rows[name] = reference_row(t, LISTS[name])
    return t, rows[name]


@pytest.mark.gpu
@pytest.mark.parametrize("null_p", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("n", SIZES)
def test_every_function_and_type_row_for_row(gpu, n, null_p):
    for name, aggs in LISTS.items():
        t, want = table_and_reference(n, null_p, name)
        out = run(gpu, whole_plan(aggs), [batches(t)])
        assert out.schema.names == [agg_name(fn, arg) for fn, arg in aggs]
        assert out_types(out) == [RESULT[fn](TYPES[arg] if arg else None) for fn, arg in aggs], name
        got = out_row(out)
        assert same_row(got, want), (name, n, null_p, got, want)


@pytest.mark.gpu
def test_more_tiles_than_the_grid_has_workgroups(gpu):
    """The reduce grid is capped at 8 workgroups per compute unit (reduce.hpp kReduceBlocksPerCu); beyond that a workgroup walks tiles b, b + G, ...
    (cap + 1) * 8192 + 4099 rows of one Int32 column, valid in a few thousand rows spread over every part of it (the last tiles and the ragged end
    among them).  The reference skips a NULL row without touching its state, so over the valid rows alone it returns what it returns over all of them;
    COUNT(*) counts every row."""
    import torch
    cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    n = (cap + 1) * TILE + 4099
    r = np.random.default_rng(5)
    v = r.integers(-2**31, 2**31 - 1, n, dtype=np.int32)
    ok = np.zeros(n, bool)
    ok[r.integers(0, n, 6000)] = True
    ok[cap * TILE - 3:cap * TILE + 5] = True        # either side of the first tile a workgroup takes as its second
    ok[n - 4101:n - 4095] = True                     # ... and of the start of the ragged tile
    ok[n - 3:] = True
    aggs = SIX("i")
    dense = {"i": (v[ok], np.ones(int(ok.sum()), bool))}
    assert reference_is_exact(dense, aggs, SUM_RANGE)
    want = reference_row(dense, aggs)
    want[0] = n
    out = run(gpu, whole_plan(aggs, cols=[("i", "Int32")]), [[pa.record_batch([pa.array(v, mask=~ok)], names=["i"])]])
    assert same_row(out_row(out), want), (out_row(out), want)


@pytest.mark.gpu
def test_null_rows_are_dropped_only_where_every_aggregate_skips_them(gpu):
    """COUNT(*), MAX(i): i's NULL rows are counted (copying the lone MAX's feed-time dropping would miscount); SUM(i), COUNT(l): a row whose i is NULL
    still counts for l; MIN(i), MAX(i): whether the leaf drops the rows or the kernel skips them, the row is the same."""
    t = make_table(TILE + 77, 97, 0.3)
    for aggs in ([("count", None), ("max", "i")], [("sum", "i"), ("count", "l")], [("min", "i"), ("max", "i")], [("count", "i")]):
        assert reference_is_exact(t, aggs, SUM_RANGE)
        assert same_row(out_row(run(gpu, whole_plan(aggs), [batches(t, 2)])), reference_row(t, aggs)), aggs


# ------------------------------------------------------------------ GPU 2: modes
MODE_AGGS = [("count", None), ("count", "l"), ("sum", "l"), ("min", "l"), ("max", "t"), ("avg", "i"), ("min", "f")]


def _state_cols(aggs):
    return [(f["name"], "ts" if f["data_type"] == _TS else f["data_type"]) for f in state_fields(aggs)]


def _state_batch(rows, aggs):
    cols = _state_cols(aggs)
    arrs = []
    for k, (name, ty) in enumerate(cols):
        vals = [r[k] for r in rows]
        arrs.append(pa.array(vals, pa.int64()).cast(_PA[ty]) if ty == "ts" else pa.array(vals, _PA[ty]))
    return pa.record_batch(arrs, names=[c for c, _ in cols])


@pytest.mark.gpu
@pytest.mark.parametrize("n,null_p", [(0, 0.0), (5 * TILE + 4099, 0.3), (TILE + 1, 1.0)])
def test_partial_alone_emits_the_state_row(gpu, n, null_p):
    t = make_table(n, 31, null_p)
    assert reference_is_exact(t, MODE_AGGS, SUM_RANGE)
    out = run(gpu, agg_node("Partial", MODE_AGGS, _scan(NUMERIC), NUMERIC), [batches(t, 2)])
    assert out.schema.names == [f["name"] for f in state_fields(MODE_AGGS)]
    assert out_types(out) == [ty for _, ty in _state_cols(MODE_AGGS)]
    assert same_row(out_row(out), partial_state(t, MODE_AGGS))


@pytest.mark.gpu
@pytest.mark.parametrize("parts", [1, 3, 8])
def test_final_over_partial_rows(gpu, parts):
    """Final over P state rows, some of them the state of an EMPTY partition (COUNT 0, the rest NULL, AVG (0, 0.0)); with one partition, that is the only row."""
    t = make_table(3 * TILE + 77, 37, 0.3)
    n = len(t["l"][0])
    cuts = [0] + sorted(np.random.default_rng(parts).integers(0, n, parts - 1).tolist()) + [n] if parts > 1 else [0, 0]
    if parts == 8:
        cuts[3] = cuts[2]            # an empty partition in the middle
    pieces = [{c: (v[a:b], ok[a:b]) for c, (v, ok) in t.items()} for a, b in zip(cuts[:-1], cuts[1:])]
    rows = [partial_state(p, MODE_AGGS) for p in pieces]
    merged = {c: (np.concatenate([p[c][0] for p in pieces]), np.concatenate([p[c][1] for p in pieces])) for c in t}
    assert reference_is_exact(merged, MODE_AGGS, SUM_RANGE)
    want = reference_row(merged, MODE_AGGS)
    scols = _state_cols(MODE_AGGS)
    plan = agg_node("Final", MODE_AGGS, _scan(scols), NUMERIC)
    out = run(gpu, plan, [[_state_batch(rows, MODE_AGGS)]])
    assert out.schema.names == [agg_name(fn, arg) for fn, arg in MODE_AGGS]
    assert same_row(out_row(out), want), (out_row(out), want)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["host_batches", "on_device"])
def test_staged_equals_whole_equals_reference(gpu, how):
    from flock_amd import stages as S
    t = make_table(5 * TILE + 4099, 41, 0.3)
    assert reference_is_exact(t, MODE_AGGS, SUM_RANGE)
    want = reference_row(t, MODE_AGGS)
    plan = whole_plan(MODE_AGGS, cols=NUMERIC)
    assert same_row(out_row(run(gpu, plan, [batches(t, 3)])), want)
    stages = S.build_query_dag(plan)
    assert len(stages) == 2
    kw = dict(chunks=3) if how == "host_batches" else dict(on_device=True)
    staged = S.StagedRun(gpu, stages, **kw)
    try:
        out = staged.run({"t": record_batch(t)})
    finally:
        staged.close()
    out = out if isinstance(out, list) else [out]
    assert len(out) == 1 and same_row(out_row(out[0]), want), (out_row(out[0]), want)


# ------------------------------------------------------------------ GPU 3: over a filter
FCOLS = NUMERIC + [("s", "Utf8")]
WORDS = ["", "a", "abc", "xabcx", "ab", "b" * 20 + "abc"]
PREDS = {
    "leaf": lambda: _bin(_bin(_c("i", FCOLS), "Modulo", _lit("Int32", 7)), "Eq", _lit("Int32", 1)),
    "general": lambda: _bin(_bin(_c("l", FCOLS), "Divide", _lit("Int64", 100)), "Gt", _lit("Int64", 5)),
    "like": lambda: _bin(_c("s", FCOLS), "Like", _lit("Utf8", "%abc%")),
    "none": lambda: _bin(_c("l", FCOLS), "Gt", _lit("Int64", 10**15)),
    "all": lambda: _bin({"physical_expr": "is_null_expr", "arg": _c("i", FCOLS)}, "Or", {"physical_expr": "is_not_null_expr", "arg": _c("i", FCOLS)}),
}


def _filter_table(n, seed):
    t = make_table(n, seed, 0.3)
    r = np.random.default_rng(seed + 1)
    t["s"] = (np.array([WORDS[k] for k in r.integers(0, len(WORDS), n)], object), r.random(n) >= 0.2)
    return t


def _keep(t, which):
    i, l, p, s = t["i"], t["l"], t["p"], t["s"]
    if which == "leaf":      # (i % 7 = 1: the sign of the dividend, as Arrow's and C's)
        return i[1] & (np.fmod(i[0].astype(np.int64), 7) == 1)
    if which == "general":   # (l / 100 > 5, the division truncating toward zero: l >= 600)
        return l[1] & (l[0] >= 600)
    if which == "like":
        return s[1] & np.array(["abc" in x for x in s[0].tolist()], bool)
    return np.zeros(len(p[0]), bool) if which == "none" else np.ones(len(p[0]), bool)


FILTER_AGGS = [("count", None), ("count", "l"), ("sum", "i"), ("min", "l"), ("max", "t"), ("avg", "l"), ("max", "f")]


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(PREDS))
def test_over_a_filter_reads_the_input_under_the_flags(gpu, which):
    from flock_amd.runtime import ExecutionContext, collect
    t = _filter_table(5 * TILE + 4099, 53)
    keep = _keep(t, which)
    assert {"none": keep.sum() == 0, "all": keep.all()}.get(which, 0 < keep.sum() < len(keep))
    kept = {c: (v[keep], ok[keep]) for c, (v, ok) in t.items() if c != "s"}
    assert reference_is_exact(kept, FILTER_AGGS, SUM_RANGE)
    want = reference_row(kept, FILTER_AGGS)
    plan = whole_plan(FILTER_AGGS, _filter(_scan(FCOLS), PREDS[which]()), FCOLS)
    ctx = ExecutionContext([plan], gpu=gpu)
    gpu.profile_reset()
    gpu.profile(True)
    try:
        out = collect(ctx, [[batches(t, 2, FCOLS)]])[0]
        ran = gpu.profile_read()
    finally:
        gpu.profile(False)
        ctx.close()
    assert len(out) == 1 and same_row(out_row(out[0]), want), (which, out_row(out[0]), want)
    assert ("valprog_kernel" if which == "general" else "pred_flag_kernel") in ran, sorted(ran)
    assert "global_reduce_kernel" in ran and "global_fold_kernel" in ran, sorted(ran)
    for k in ran:
        assert not any(w in k for w in ("tile_scan", "emit", "gather", "take")), sorted(ran)


@pytest.mark.gpu
def test_count_star_over_a_filter_streams_nothing(gpu):
    from flock_amd.runtime import ExecutionContext, collect
    t = _filter_table(5 * TILE + 4099, 59)
    # (the Partial alone: a Final above it streams the one state row it is handed)
    plan = agg_node("Partial", [("count", None)], _filter(_scan(FCOLS), PREDS["leaf"]()), FCOLS)
    ctx = ExecutionContext([plan], gpu=gpu)
    gpu.profile_reset()
    gpu.profile(True)
    try:
        out = collect(ctx, [[batches(t, 1, FCOLS)]])[0]
        ran = gpu.profile_read()
    finally:
        gpu.profile(False)
        ctx.close()
    assert out_row(out[0]) == [int(_keep(t, "leaf").sum())]
    assert "pred_flag_kernel" in ran and "global_fold_kernel" in ran and "global_reduce_kernel" not in ran, sorted(ran)


@pytest.mark.gpu
def test_computed_argument_over_a_filter_is_correct(gpu):
    """SUM(i * 2), COUNT(*) over a filter: the argument's projection sits between the aggregate and the filter -- the ordinary, materialising route."""
    t = _filter_table(2 * TILE + 17, 61)
    keep = _keep(t, "leaf")
    kept = {"x": (t["i"][0][keep].astype(np.int64) * 2, t["i"][1][keep])}
    want = reference_row(kept, [("sum", "x"), ("count", None)])
    e = _bin({"physical_expr": "cast_expr", "expr": _c("i", FCOLS), "cast_type": "Int64"}, "Multiply", _lit("Int64", 2))
    entries = [_entry("sum", None, FCOLS, expr=e, ty="Int64"), _entry("count", None, FCOLS)]
    inner = agg_node("Partial", None, _filter(_scan(FCOLS), PREDS["leaf"]()), FCOLS, entries=entries)
    plan = agg_node("Final", None, {"execution_plan": "coalesce_partitions_exec", "input": inner}, FCOLS, entries=entries)
    assert same_row(out_row(run(gpu, plan, [batches(t, 1, FCOLS)])), want)


# ------------------------------------------------------------------ GPU 4: shape independence
@pytest.mark.gpu
def test_batches_and_repeats_change_no_bit(gpu):
    from flock_amd.runtime import ExecutionContext, collect
    t = make_table(5 * TILE + 4099, 67, 0.3)
    aggs = [("max", "t"), ("sum", "i"), ("count", None), ("avg", "l"), ("min", "f"), ("avg", "u")]     # (eight accumulators: AVG takes two)
    assert reference_is_exact(t, aggs, SUM_RANGE)
    plan = whole_plan(aggs)
    seen = set()
    for k in (1, 3, 17):
        ctx = ExecutionContext([plan], gpu=gpu)
        try:
            for _ in range(2):       # (the second execute finds the first one's arenas)
                out = collect(ctx, [[batches(t, k)]])[0]
                assert len(out) == 1 and out[0].num_rows == 1
                seen.add(row_bits(out_row(out[0])))
        finally:
            ctx.close()
    assert len(seen) == 1, seen
    assert seen == {row_bits(reference_row(t, aggs))}


# ------------------------------------------------------------------ GPU 5: above and below other operators
def _group_by(inp, key, cols):
    cnt = _entry("count", None, cols)
    pf = [_field(key, dict(cols)[key]), _field("COUNT(UInt8(1))[count]", "UInt64")]
    part = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [[_c(key, cols), key]], "aggr_expr": [cnt], "input": inp,
            "input_schema": {"fields": [_field(n, t) for n, t in cols], "metadata": {}}, "schema": {"fields": pf, "metadata": {}}}
    rep = {"execution_plan": "repartition_exec", "input": part, "partitioning": {"Hash": [[{"physical_expr": "column", "name": key, "index": 0}], 4]}}
    return {"execution_plan": "hash_aggregate_exec", "mode": "FinalPartitioned", "group_expr": [[{"physical_expr": "column", "name": key, "index": 0}, key]],
            "aggr_expr": [cnt], "input": rep, "input_schema": {"fields": [_field(n, t) for n, t in cols], "metadata": {}}, "schema": {"fields": [], "metadata": {}}}


@pytest.mark.gpu
def test_over_a_group_bys_output(gpu):
    """q5's shape with two aggregates: MAX(n), COUNT(*) over (p, COUNT(*) AS n)"""
    t = make_table(3 * TILE + 5, 71, 0.0)
    t["p"] = (np.random.default_rng(3).integers(0, 500, len(t["i"][0])).astype(np.int32), np.ones(len(t["i"][0]), bool))
    gcols = [("p", "Int32"), ("COUNT(UInt8(1))", "UInt64")]
    top = [_entry("max", "COUNT(UInt8(1))", gcols), _entry("count", None, gcols)]
    inner = agg_node("Partial", None, _group_by(_scan(NUMERIC), "p", NUMERIC), gcols, entries=top)
    plan = agg_node("Final", None, {"execution_plan": "coalesce_partitions_exec", "input": inner}, gcols, entries=top)
    counts = np.bincount(t["p"][0])
    counts = counts[counts > 0]
    want = reference_row({"n": (counts.astype(np.uint64), np.ones(len(counts), bool))}, [("max", "n"), ("count", None)])
    assert out_row(run(gpu, plan, [batches(t, 2)])) == want


@pytest.mark.gpu
@pytest.mark.parametrize("null_row", [False, True])
def test_as_the_right_side_of_an_inner_join(gpu, null_row):
    """q7's shape: rows JOIN (SELECT MAX(l), COUNT(*) ...) ON l = MAX(l) -- and over an all-NULL column the one row's key is NULL and matches nothing."""
    t = make_table(TILE + 9, 73, 1.0 if null_row else 0.3)
    rt = make_table(300, 79, 0.0, cols=[("l", "Int64")])
    rt["l"][0][:] = np.arange(300) - 150
    if not null_row:
        mx = int(t["l"][0][t["l"][1]].max())
        rt["l"][0][7] = rt["l"][0][200] = mx
    lcols, acols = [("l_l", "Int64")], [("MAX(l)", "Int64"), ("COUNT(UInt8(1))", "UInt64")]
    left = {"execution_plan": "memory_exec", "schema": {"fields": [_field("l_l", "Int64")], "metadata": {}}, "projection": [0]}
    join = {"execution_plan": "hash_join_exec", "left": left, "right": whole_plan([("max", "l"), ("count", None)], cols=NUMERIC), "join_type": "Inner", "mode": "CollectLeft",
            "on": [[_c("l_l", lcols), _c("MAX(l)", acols)]], "schema": {"fields": [_field(n, ty) for n, ty in lcols + acols], "metadata": {}}}
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([join], gpu=gpu)
    try:
        out = collect(ctx, [[[pa.record_batch([pa.array(rt["l"][0])], names=["l_l"])]], [batches(t)]])[0]
    finally:
        ctx.close()
    rows = sorted(r for b in out for r in zip(*[c.to_pylist() for c in b.columns]))
    n = len(t["l"][0])
    assert rows == ([] if null_row else [(mx, mx, n), (mx, mx, n)])


@pytest.mark.gpu
def test_over_a_semi_join_and_over_sort_limit(gpu):
    t = make_table(2 * TILE + 100, 83, 0.3)
    n = len(t["l"][0])
    rt = {"l_r": (t["l"][0][::3].copy(), np.ones(len(t["l"][0][::3]), bool))}
    rcols = [("l_r", "Int64")]
    semi = {"execution_plan": "hash_join_exec", "left": _scan(NUMERIC), "right": _scan(rcols), "join_type": "Semi", "mode": "CollectLeft",
            "on": [[_c("l", NUMERIC), _c("l_r", rcols)]], "schema": {"fields": [_field(c, ty) for c, ty in NUMERIC], "metadata": {}}}
    aggs = [("count", None), ("sum", "i"), ("max", "t"), ("avg", "l")]
    keep = t["l"][1] & np.isin(t["l"][0], rt["l_r"][0])
    kept = {c: (v[keep], ok[keep]) for c, (v, ok) in t.items()}
    assert reference_is_exact(kept, aggs, SUM_RANGE) and 0 < keep.sum() < n
    out = run(gpu, whole_plan(aggs, semi, NUMERIC), [batches(t), [record_batch(rt, cols=rcols)]])
    assert same_row(out_row(out), reference_row(kept, aggs))
    # ORDER BY p DESC LIMIT 500 (p without NULLs, ties in input order), then the aggregates
    t["p"] = (np.random.default_rng(9).integers(0, 10**6, n).astype(np.int32), np.ones(n, bool))
    sort = {"execution_plan": "sort_exec", "input": _scan(NUMERIC), "expr": [{"expr": _c("p", NUMERIC), "options": {"descending": True, "nulls_first": False}}]}
    lim = {"execution_plan": "global_limit_exec", "input": sort, "limit": 500}
    top = np.argsort(-t["p"][0].astype(np.int64), kind="stable")[:500]
    kept = {c: (v[top], ok[top]) for c, (v, ok) in t.items()}
    assert reference_is_exact(kept, aggs, SUM_RANGE)
    assert same_row(out_row(run(gpu, whole_plan(aggs, lim, NUMERIC), [batches(t)])), reference_row(kept, aggs))


@pytest.mark.gpu
def test_an_empty_relation_gives_one_row_never_an_empty_batch(gpu):
    """tests/test_plan_round5b.py test_the_new_operators_on_an_empty_relation says an ungrouped aggregate over nothing is one row: so are the new functions, in
    every mode, over a scan and over a filter, twice (the second execute finds the first one's arenas)."""
    from flock_amd.runtime import ExecutionContext, collect
    t = _filter_table(0, 89)
    aggs = FILTER_AGGS
    want = reference_row({c: v for c, v in t.items() if c != "s"}, aggs)
    assert want == [0, 0, None, None, None, None, None]
    for plan in (whole_plan(aggs, cols=FCOLS), whole_plan(aggs, _filter(_scan(FCOLS), PREDS["general"]()), FCOLS), agg_node("Partial", aggs, _scan(FCOLS), FCOLS)):
        ctx = ExecutionContext([plan], gpu=gpu)
        try:
            for _ in range(2):
                out = collect(ctx, [[batches(t, 1, FCOLS)]])[0]
                assert len(out) == 1 and out[0].num_rows == 1
                if plan["mode"] == "Final":
                    assert out_row(out[0]) == want
                else:
                    assert out_row(out[0]) == partial_state({c: v for c, v in t.items() if c != "s"}, aggs)
        finally:
            ctx.close()
