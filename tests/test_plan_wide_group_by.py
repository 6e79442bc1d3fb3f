"""GROUP BY with five to sixteen accumulators per node (flock_amd/csrc/groupwide.hpp; NEXMark q17's auction statistics carry nine): every key shape, Partial /
Final / FinalPartitioned, stage plans, the tile and LDS-bin edges of the pass -- row multisets against the plain-Python reference of tests/wide_group_ref.py,
which a CPU test holds to pyarrow's Table.group_by.  A plan of at most four accumulators keeps its path and its group order."""
import json
import os

import numpy as np
import pyarrow as pa
import pytest

import wide_group_ref as ref
from wide_group_ref import agg_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")

TS = {"Timestamp": ["Millisecond", None]}
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string(), "ts": pa.timestamp("ms")}
# keys: kd dense Int32, kw Int64 scattered over 2^40, ks Utf8, kn Int32 with NULL keys, kt Timestamp, k2 Int64 with NULL keys; arguments: the rest
COLS = [("kd", "Int32"), ("kw", "Int64"), ("ks", "Utf8"), ("kn", "Int32"), ("kt", "ts"), ("k2", "Int64"),
        ("i", "Int32"), ("l", "Int64"), ("u", "UInt64"), ("t", "ts"), ("f", "Float64"), ("i2", "Int32"), ("l2", "Int64"), ("j", "Int32"),
        ("i3", "Int32"), ("l3", "Int64"), ("t3", "ts")]
TYPES = dict(COLS)
ARGS = ["i", "l", "u", "t", "f", "i2", "l2", "j"]
SIXTEEN = ARGS + ["i3", "l3", "t3", "kd", "kw", "kn", "kt", "k2"]      # sixteen distinct argument columns: the most one node takes (every accumulator its own)
TILE = 8192
BINS = {8: 448, 16: 224}                                # groupwide.hpp wide_group_bins: five to eight accumulators, nine to sixteen
RESULT = {"dc": lambda t: "UInt64", "count": lambda t: "UInt64", "avg": lambda t: "Float64", "sum": lambda t: "UInt64" if t == "UInt64" else "Int64", "min": lambda t: t,
          "max": lambda t: t}

# accumulator lists (AVG takes two)
A5 = [("count", None), ("sum", "i"), ("min", "l"), ("max", "u"), ("count", "l")]
A8 = [("avg", "i"), ("count", None), ("min", "t"), ("max", "f"), ("sum", "l"), ("min", "i"), ("max", "i")]                          # AVG first
A9 = [("count", None), ("count", "i"), ("count", "l"), ("count", "t"), ("min", "i"), ("max", "i"), ("avg", "i"), ("sum", "i")]      # q17's list
A16_ONE = [(fn, "l") for fn in ("sum", "min", "max", "count", "avg")] * 2 + [(fn, "l") for fn in ("sum", "min", "max", "count")]     # sixteen over ONE column
A16_EIGHT = [(fn, c) for c in ARGS for fn in ("min", "max")]                                                                        # ... over eight
A16_SIXTEEN = [("max" if k % 2 else "min", c) for k, c in enumerate(SIXTEEN)]                                                         # ... over sixteen
A16_AVG_LAST = [(fn, c) for c in ARGS[:7] for fn in ("min", "max")] + [("avg", "j")]                                                # AVG last
# (the AVGs over columns whose sums stay below 2^53: a Partial's sum state is a double, and Final adds the states of several Partials)
A16_SUMS = [("sum", "i"), ("sum", "l"), ("sum", "u"), ("avg", "i"), ("avg", "i2"), ("avg", "j"), ("min", "f"), ("max", "f"), ("count", "f"), ("count", None),
            ("min", "u"), ("max", "t"), ("sum", "i2")]
LISTS = {"a5": A5, "a8": A8, "a9": A9, "a16_one": A16_ONE, "a16_eight": A16_EIGHT, "a16_sixteen": A16_SIXTEEN, "a16_avg_last": A16_AVG_LAST, "a16_sums": A16_SUMS}


def n_accs(aggs):
    return sum(0 if fn == "dc" else 2 if fn == "avg" else 1 for fn, _ in aggs)


assert [n_accs(LISTS[k]) for k in ("a5", "a8", "a9", "a16_one", "a16_eight", "a16_sixteen", "a16_avg_last", "a16_sums")] == [5, 8, 9, 16, 16, 16, 16, 16]


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


def _entry(i, fn, arg, cols=COLS, expr=None, ty=None):
    at = dict(cols)[arg] if arg in dict(cols) else None
    e = expr if expr is not None else (_c(arg, cols) if arg else _lit("UInt8", 1))
    if fn == "dc":
        return {"aggregate_expr": "distinct_count", "name": agg_name(i, fn, arg), "data_type": "UInt64", "nullable": True, "exprs": [e], "state_data_types": [_dt(at)],
                "input_data_types": [_dt(at)]}
    return {"aggregate_expr": fn, "name": agg_name(i, fn, arg), "data_type": _dt(ty or RESULT[fn](at)), "nullable": True, "expr": e}


def _list_field(name, t):
    item = {"data_type": _dt(t), "dict_id": 0, "dict_is_ordered": False, "name": "item", "nullable": True}
    return {"data_type": {"List": item}, "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": False}


def state_cols(aggs, cols=COLS, types=None):
    """(name, type) of the state columns a Partial writes for `aggs`; types: per entry, the argument's type where it is computed"""
    out = []
    for i, (fn, arg) in enumerate(aggs):
        name, at = agg_name(i, fn, arg), (types or {}).get(i, dict(cols).get(arg))
        if fn == "avg":
            out += [(name + "[count]", "UInt64"), (name + "[sum]", "Float64")]
        else:
            out.append(("%s[%s]" % (name, fn), RESULT[fn](at)))
    return out


def agg_node(mode, keys, aggs, inp, cols=COLS, entries=None, types=None):
    """One hash_aggregate_exec.  Partial: the group keys are the input's columns; Final: the Partial's, by position."""
    entries = entries if entries is not None else [_entry(i, fn, arg, cols) for i, (fn, arg) in enumerate(aggs)]
    group = [[_c(k, cols) if mode == "Partial" else {"physical_expr": "column", "name": k, "index": i}, k] for i, k in enumerate(keys)]
    kf = [_field(k, dict(cols)[k]) for k in keys]
    if mode == "Partial":
        fields = kf + [_list_field(n, "Int32") if n.endswith("[dc]") else _field(n, t) for n, t in state_cols(aggs, cols, types)]
    else:
        fields = kf + [_field(agg_name(i, fn, arg), RESULT[fn]((types or {}).get(i, dict(cols).get(arg)))) for i, (fn, arg) in enumerate(aggs)]
    return {"execution_plan": "hash_aggregate_exec", "mode": mode, "group_expr": group, "aggr_expr": entries, "input": inp,
            "input_schema": {"fields": [_field(n, t) for n, t in cols], "metadata": {}}, "schema": {"fields": fields, "metadata": {}}}


def whole_plan(keys, aggs, inp=None, cols=COLS, mode="FinalPartitioned", entries=None, parts=4, types=None):
    """Partial -> Hash repartition on the keys -> Final*, as the planner writes SELECT <keys>, <aggs> FROM ... GROUP BY <keys>"""
    partial = agg_node("Partial", keys, aggs, inp or _scan(cols), cols, entries, types)
    mid = {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096,
           "input": {"execution_plan": "repartition_exec", "input": partial,
                     "partitioning": {"Hash": [[{"physical_expr": "column", "name": k, "index": i} for i, k in enumerate(keys)], parts]}}}
    return agg_node(mode, keys, aggs, mid, cols, entries, types)


# ------------------------------------------------------------------ tables: {column: [values, None = NULL]}
def make_table(n, seed, null_p=0.0, groups=37, ids="scattered"):
    """ids -- how the rows name their groups: "scattered" at random; "cycle" row r names group r % groups (one tile spans every id); "runs" ascending runs of
    equal ids; "hot" one group on half the rows; "switch" the same, the hot group changing at row 1000 -- inside one 256-row access of a wave.
    Values: Int64 near +-2^62 (a group's SUM wraps), UInt64 at and above 2^63, Float64 with negative values, -0.0 and +0.0, Int32 over its whole range."""
    r = np.random.default_rng(seed)
    if ids == "cycle":
        g = np.arange(n, dtype=np.int64) % groups
    elif ids == "runs":
        g = np.arange(n, dtype=np.int64) * groups // max(n, 1)
    elif ids in ("hot", "switch"):
        hot = np.where(np.arange(n) < 1000, 3, 5) % groups if ids == "switch" else np.zeros(n, np.int64)
        g = np.where(r.random(n) < 0.5, hot, r.integers(0, groups, n)).astype(np.int64)
    else:
        g = r.integers(0, groups, n).astype(np.int64)
    t = {}
    t["kd"] = (g + 100).tolist()
    t["kw"] = ((g * 0x9E3779B1) % (1 << 40) - (1 << 39)).tolist()
    t["ks"] = ["key-%d" % k if k else "" for k in g.tolist()]
    t["kn"] = [None if k == 1 else k for k in g.tolist()]
    t["kt"] = (1_436_918_400_000 + (g % 7) * 86_400_000).tolist()
    t["k2"] = [None if k % 5 == 2 else k // 5 * 10**12 for k in g.tolist()]
    t["i"] = r.integers(-2**31, 2**31, n).tolist()
    t["l"] = (r.integers(-3, 4, n) * 2**61 + r.integers(-1000, 1000, n)).tolist()
    t["u"] = [2**63 - 5 + int(v) for v in r.integers(0, 2**40, n).tolist()]
    t["t"] = (1_436_918_400_000 + r.integers(-10**9, 10**9, n)).tolist()
    t["f"] = [[-0.0, 0.0, -1.5, 2.25][int(v)] if v < 4 else float(v - 40) * 0.37 for v in r.integers(0, 80, n).tolist()]
    t["i2"] = r.integers(-50, 50, n).tolist()
    t["l2"] = r.integers(-10**15, 10**15, n).tolist()
    t["j"] = r.integers(0, 10**6, n).tolist()
    t["i3"] = r.integers(-9, 9, n).tolist()
    t["l3"] = r.integers(-2**62, 2**62, n).tolist()
    t["t3"] = (1_436_918_400_000 + r.integers(0, 10**7, n)).tolist()
    if null_p > 0:
        for c in ARGS + ["i3", "l3", "t3"]:
            ok = r.random(n) >= null_p
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


def want_rows(t, keys, aggs):
    return ref.sort_rows(ref.aggregate(t, keys, aggs, TYPES), len(keys))


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


def check(gpu, t, keys, aggs, k=1, want=None, **kw):
    out = run(gpu, whole_plan(keys, aggs, **kw), [batches(t, k)])
    want = want if want is not None else want_rows(t, keys, aggs)
    got = ref.sort_rows(out_rows(out), len(keys))
    assert ref.same_rows(got, want), (keys, aggs, len(got), len(want), [p for p in zip(got, want) if p[0] != p[1]][:3])
    for rb in out:
        assert rb.schema.names == list(keys) + [agg_name(i, fn, arg) for i, (fn, arg) in enumerate(aggs)]
        assert [f.type for f in rb.schema][len(keys):] == [_PA[RESULT[fn](TYPES[arg] if arg else None)] for fn, arg in aggs]
    return got


_tables, _wants = {}, {}


def table(n, null_p=0.15, groups=37, ids="scattered"):
    """One table per shape: built once, shared, never changed."""
    key = (n, null_p, groups, ids)
    if key not in _tables:
        _tables[key] = make_table(n, 17 + n % 977 + groups + len(ids), null_p, groups, ids)
    return _tables[key]


def wanted(tkey, keys, aggs):
    """the reference's rows for table(*tkey), computed once per (table, keys, list)"""
    key = (tkey, tuple(keys), tuple(aggs))
    if key not in _wants:
        _wants[key] = want_rows(table(*tkey), keys, aggs)
    return _wants[key]


# ------------------------------------------------------------------ CPU: the reference
def test_reference_on_hand_worked_rows():
    t = {"g": [1, 1, 2, 2, None, None, 3], "v": [5, -7, None, 7, 8, 8, None], "f": [-0.0, 0.0, -2.5, None, 1.0, None, None],
         "l": [2**62, 2**62, 2**63 - 1, 1, None, None, None], "u": [2**63, 2**63, 1, None, 2**64 - 1, 1, None]}
    aggs = [("count", None), ("count", "v"), ("sum", "v"), ("min", "v"), ("max", "v"), ("avg", "v")]
    assert ref.sort_rows(ref.aggregate(t, ["g"], aggs), 1) == [(None, 2, 2, 16, 8, 8, 8.0), (1, 2, 2, -2, -7, 5, -1.0), (2, 2, 1, 7, 7, 7, 7.0), (3, 1, 0, None, None, None, None)]
    got = ref.sort_rows(ref.aggregate(t, ["g"], [("min", "f"), ("max", "f")]), 1)
    assert ref.same_rows(got, [(None, 1.0, 1.0), (1, -0.0, 0.0), (2, -2.5, -2.5), (3, None, None)])
    assert not ref.same_rows([(0.0,)], [(-0.0,)])
    # SUM wraps in 64 bits: signed for Int64, modulo 2^64 for UInt64
    assert ref.sort_rows(ref.aggregate(t, ["g"], [("sum", "l"), ("sum", "u")], {"l": "Int64", "u": "UInt64"}), 1) == [(None, None, 0), (1, -2**63, 0), (2, -2**63, 1), (3, None, None)]
    assert ref.aggregate({"g": [], "v": []}, ["g"], aggs) == []


@pytest.mark.parametrize("seed", [1, 2])
def test_reference_against_pyarrow(seed):
    t = make_table(3000, seed, 0.3)
    t["l"] = [None if v is None else v // 2**50 for v in t["l"]]      # (pyarrow's checked sum does not wrap: a column whose sums fit)
    t["f"] = [None if v is None else v + 0.125 for v in t["f"]]       # (no zero of either sign: pyarrow's choice between them is its own)
    tab = pa.Table.from_batches([record_batch(t)])
    fns = {"count": "count", "sum": "sum", "min": "min", "max": "max", "avg": "mean"}
    for keys in (["kd"], ["kn"], ["ks"], ["kd", "kt"], ["ks", "kn", "k2"]):
        for arg in ("i", "l", "j", "f", "t"):
            use = [fn for fn in fns if not (arg == "f" and fn in ("sum", "avg")) and not (arg == "t" and fn in ("sum", "avg"))]
            got = tab.group_by(keys, use_threads=False).aggregate([(arg, fns[fn]) for fn in use] + [([], "count_all")])
            cols = [got.column(k) for k in keys] + [got.column("%s_%s" % (arg, fns[fn])) for fn in use] + [got.column("count_all")]
            rows = list(zip(*[(c.cast(pa.int64()) if pa.types.is_timestamp(c.type) else c).to_pylist() for c in cols]))
            want = ref.aggregate(t, keys, [(fn, arg) for fn in use] + [("count", None)], TYPES)
            assert ref.sort_rows(rows, len(keys)) == ref.sort_rows(want, len(keys)), (keys, arg)


# ------------------------------------------------------------------ CPU: explain, refusals, the fixture
def _refused(plan, *words):
    from flock_amd import FlockGpuError
    from flock_amd.runtime import explain
    with pytest.raises(FlockGpuError) as e:
        explain(plan)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


Q17_COLUMNS = ["auction:Int32", "day:Timestamp(ms)", "total_bids:UInt64", "rank1_bids:UInt64", "rank2_bids:UInt64", "rank3_bids:UInt64", "MIN(price):Int32",
               "MAX(price):Int32", "AVG(price):Float64", "SUM(price):Int64"]


def test_q17_explains_with_its_ten_columns():
    from flock_amd.runtime import explain
    text = explain(open(os.path.join(PLANS, "q17_auction_stats.json")).read())
    first = text.splitlines()[0]
    assert first.startswith("Aggregate(FinalPartitioned) [" + ", ".join(Q17_COLUMNS) + "]"), text
    assert "date_trunc('day', b_date_time)" in text and "Aggregate(Partial)" in text, text


def test_sixteen_accumulators_explain_and_seventeen_are_refused_at_explain():
    from flock_amd.runtime import explain
    for name in ("a16_one", "a16_eight", "a16_sixteen", "a16_avg_last", "a16_sums"):
        for keys in (["kd"], ["ks", "kd", "kw"]):
            first = explain(whole_plan(keys, LISTS[name])).splitlines()[0]
            assert first.startswith("Aggregate(FinalPartitioned) [") and first.count(":") >= len(keys) + len(LISTS[name]), first
    for aggs in (A16_EIGHT + [("count", None)], A16_ONE + [("max", "i")], A16_AVG_LAST[:-1] + [("avg", "j"), ("avg", "i")], [("avg", c) for c in "iljt"] * 2 + [("sum", "i")]):
        assert n_accs(aggs) > 16
        _refused(whole_plan(["kd"], aggs), "more than 16 accumulators in one GROUP BY")
        _refused(agg_node("Partial", ["kd", "ks"], aggs, _scan()), "more than 16 accumulators in one GROUP BY")
    # distinct counts take no accumulator: sixteen beside two of them explain
    assert "single pass" in explain(whole_plan(["kd"], A16_EIGHT + [("dc", "i"), ("dc", "l")]))


def test_the_other_limits_keep_their_words():
    five = [("dc", c) for c in ("i", "l", "u", "t", "j")]
    _refused(whole_plan(["kd"], five + A5), "more than 4 distinct counts")
    ungrouped = [(fn, c) for c in "il" for fn in ("count", "sum", "min", "max")] + [("count", None)]
    part = agg_node("Partial", [], ungrouped, _scan())
    final = agg_node("Final", [], ungrouped, {"execution_plan": "coalesce_partitions_exec", "input": part})
    _refused(final, "more than 8 accumulators in one ungrouped aggregate")


def test_q17_splits_into_stages_that_explain():
    from flock_amd.runtime import explain
    from flock_amd.stages import build_query_dag
    stages = build_query_dag(json.load(open(os.path.join(PLANS, "q17_auction_stats.json"))))
    assert len(stages) == 2 and stages[0].is_shuffling
    first = explain(stages[0].plan)
    assert "Aggregate(Partial)" in first and "AVG(price)[count]:UInt64" in first and "AVG(price)[sum]:Float64" in first, first
    last = explain(stages[1].plan).splitlines()[0]
    assert last.startswith("Aggregate(FinalPartitioned) [" + ", ".join(Q17_COLUMNS) + "]"), last


# ------------------------------------------------------------------ GPU 1: accumulator counts x row counts (the tile edges, the ragged 16-byte tail)
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
@pytest.mark.parametrize("name", ["a5", "a8", "a9", "a16_one", "a16_eight", "a16_sixteen", "a16_avg_last", "a16_sums"])
def test_accumulator_lists_over_the_tile_edges(gpu, name, n):
    check(gpu, table(n), ["kd"], LISTS[name], want=wanted((n,), ["kd"], LISTS[name]))


# ------------------------------------------------------------------ GPU 2: groups -- one, the LDS bins' edge, runs, scattered, hot
@pytest.mark.gpu
@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("name", ["a8", "a9", "a16_sixteen"])
def test_a_tile_that_spans_the_lds_bins(gpu, name, delta):
    """Row r names group r % G: every full tile spans all G ids -- G = bins - 1 and bins aggregate in LDS, bins + 1 goes to the global cells (the last tile,
    a handful of rows, takes the LDS path in every case)."""
    aggs = LISTS[name]
    groups = BINS[8 if n_accs(aggs) <= 8 else 16] + delta
    tkey = (2 * TILE + 5, 0.15, groups, "cycle")
    got = check(gpu, table(*tkey), ["kd"], aggs, want=wanted(tkey, ["kd"], aggs))
    assert len(got) == groups


@pytest.mark.gpu
@pytest.mark.parametrize("ids,groups", [("scattered", 1), ("runs", 700), ("scattered", 3000), ("hot", 900), ("switch", 40)])
def test_group_shapes(gpu, ids, groups):
    tkey = (2 * TILE + 77, 0.15, groups, ids)
    for aggs in (A9, A16_SUMS):
        check(gpu, table(*tkey), ["kd"], aggs, want=wanted(tkey, ["kd"], aggs))


# ------------------------------------------------------------------ GPU 3: types and NULLs
@pytest.mark.gpu
def test_adversarial_values(gpu):
    t = {c: [0] * 8 for c, _ in COLS}
    t["ks"] = [""] * 8
    t["kd"] = [1, 1, 1, 2, 2, 3, 3, 1]
    t["u"] = [2**63, 2**64 - 1, 2**63 + 7, 5, 1, None, None, 0]                             # a maximum above 2^63
    t["l"] = [2**62, 2**62, 2**62, -2**63, -1, None, None, 2**62]                           # group 1: 4 * 2^62 wraps to 0; group 2: -2^63 - 1 wraps to 2^63 - 1
    t["i"] = [-2**31, 2**31 - 1, None, 5, -5, None, None, 7]                                # Int32 MIN / MAX come back Int32
    t["f"] = [-0.0, 0.0, None, -2.5, -1e300, None, None, None]
    t["t"] = [1_436_918_400_000, None, 5, -5, None, None, None, 0]
    t["j"] = [None, None, None, None, None, 1, 2, None]                                     # groups 1 and 2: nothing but NULLs here, values in every other column
    aggs = [("max", "u"), ("sum", "l"), ("min", "i"), ("max", "i"), ("min", "f"), ("max", "f"), ("min", "t"), ("max", "t"), ("count", "j"), ("sum", "j"), ("avg", "j"),
            ("count", "i"), ("sum", "u")]
    got = check(gpu, t, ["kd"], aggs)
    assert ref.same_rows(got, [(1, 2**64 - 1, 0, -2**31, 2**31 - 1, -0.0, 0.0, 0, 1_436_918_400_000, 0, None, None, 3, (2**63 + 2**64 - 1 + 2**63 + 7) % 2**64),
                               (2, 5, 2**63 - 1, -5, 5, -1e300, -2.5, -5, -5, 0, None, None, 2, 6),
                               (3, None, None, None, None, None, None, None, None, 2, 3, 1.5, 0, None)])


@pytest.mark.gpu
def test_a_computed_case_argument_that_is_null_for_most_rows(gpu):
    tkey = (TILE + 1, 0.15)
    t = table(*tkey)
    # CASE WHEN j < 50000 THEN l2 END: NULL for 95 rows in 100 (and where j is NULL); COUNT, MIN and AVG of it beside plain columns
    case = {"physical_expr": "case_expr", "expr": None, "when_then_expr": [[_bin(_c("j"), "Lt", _lit("Int32", 50000)), _c("l2")]], "else_expr": None}
    aggs = [("count", "case"), ("min", "case"), ("avg", "case"), ("count", None), ("max", "i"), ("sum", "l2"), ("min", "f")]
    entries = [_entry(i, fn, arg, expr=case if arg == "case" else None, ty=None if arg != "case" else RESULT[fn]("Int64")) for i, (fn, arg) in enumerate(aggs)]
    types = {i: "Int64" for i, (fn, arg) in enumerate(aggs) if arg == "case"}
    out = run(gpu, whole_plan(["ks"], aggs, entries=entries, types=types), [batches(t, 2)])
    tc = dict(t, case=[v if jj is not None and jj < 50000 else None for v, jj in zip(t["l2"], t["j"])])
    assert sum(v is not None for v in tc["case"]) < len(tc["case"]) // 10
    assert ref.same_rows(ref.sort_rows(out_rows(out), 1), want_rows(tc, ["ks"], aggs))


@pytest.mark.gpu
def test_sum_and_avg_of_float64_stay_refused_in_todays_words(gpu):
    from flock_amd import FlockGpuError
    for fn, words in (("sum", "sum needs an integer column"), ("avg", "AVG needs an integer column")):
        with pytest.raises(FlockGpuError) as e:
            run(gpu, whole_plan(["kd"], A5 + [(fn, "f")]), [batches(table(1))])
        assert words in str(e.value), str(e.value)


# ------------------------------------------------------------------ GPU 4: key shapes
KEYS = {"dense_i32": ["kd"], "sparse_i64": ["kw"], "utf8": ["ks"], "i32_ts": ["kd", "kt"], "utf8_i32_i64": ["ks", "kd", "kw"], "null_keys": ["kn"], "null_keys_two": ["kn", "k2"]}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(KEYS))
def test_every_key_shape(gpu, shape):
    tkey = (TILE + 1, 0.15)
    for aggs in (A5, A16_SUMS):
        got = check(gpu, table(*tkey), KEYS[shape], aggs, want=wanted(tkey, KEYS[shape], aggs))
        if shape.startswith("null_keys"):
            assert got[0][0] is None      # NULL keys form one group


# ------------------------------------------------------------------ GPU 5: modes
def state_rows(t, keys, aggs):
    """what a Partial writes: COUNT -> count, SUM / MIN / MAX -> the value, AVG -> (count, double(sum))"""
    flat, avg_at = [], []
    for fn, arg in aggs:
        if fn == "avg":
            avg_at.append(len(flat) + 1)
            flat += [("count", arg), ("sum", arg)]
        else:
            flat.append((fn, arg))
    rows = []
    for r in ref.aggregate(t, keys, flat, TYPES):
        r = list(r)
        for a in avg_at:
            r[len(keys) + a] = float(r[len(keys) + a] or 0)
        rows.append(tuple(r))
    return ref.sort_rows(rows, len(keys))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a9", "a16_sums"])
def test_a_partial_alone_and_its_states_through_a_final_plan(gpu, name):
    aggs = LISTS[name]
    tkey = (TILE + 1, 0.15)
    t = table(*tkey)
    keys = ["kd", "kt"]
    states = run(gpu, agg_node("Partial", keys, aggs, _scan()), [batches(t, 2)])
    scols = [(k, TYPES[k]) for k in keys] + state_cols(aggs)
    assert states[0].schema.names == [n for n, _ in scols] and len(scols) == len(keys) + n_accs(aggs)
    assert ref.same_rows(ref.sort_rows(out_rows(states), len(keys)), state_rows(t, keys, aggs))
    # the states of two Partials (the table's halves, each grouped on its own) through FinalPartitioned and Final
    halves = [run(gpu, agg_node("Partial", keys, aggs, _scan()), [[b]])[0] for b in batches(t, 2)]
    for mode in ("FinalPartitioned", "Final"):
        final = agg_node(mode, keys, aggs, _scan(scols))
        out = run(gpu, final, [halves])
        assert ref.same_rows(ref.sort_rows(out_rows(out), len(keys)), wanted(tkey, keys, aggs))


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["eight_partitions", "one_instance_shared", "on_device"])
def test_staged_runs_equal_the_whole_plan(gpu, how):
    from flock_amd import stages as S
    tkey = (2 * TILE + 77, 0.15, 900, "hot")
    t = table(*tkey)
    keys, aggs = ["ks", "kd"], A16_SUMS
    want = wanted(tkey, keys, aggs)
    check(gpu, t, keys, aggs, parts=8, want=want)
    stages = S.build_query_dag(whole_plan(keys, aggs, parts=8))
    assert len(stages) == 2
    kw = {"eight_partitions": dict(chunks=2), "one_instance_shared": dict(instances=1, share_sources=True), "on_device": dict(on_device=True)}[how]
    staged = S.StagedRun(gpu, stages, **kw)
    try:
        out = staged.run({"events": record_batch(t)})
    finally:
        staged.close()
    out = out if isinstance(out, list) else [out]
    assert ref.same_rows(ref.sort_rows(out_rows(out), len(keys)), want)


@pytest.mark.gpu
def test_beside_two_distinct_counts(gpu):
    tkey = (TILE + 1, 0.15)
    t = table(*tkey)
    aggs = [("dc", "i2"), ("count", None), ("avg", "i"), ("min", "f"), ("dc", "j"), ("max", "u"), ("sum", "l"), ("count", "t")]
    got = ref.sort_rows(out_rows(run(gpu, whole_plan(["kd"], aggs), [batches(t, 2)])), 1)
    plain = [a for a in aggs if a[0] != "dc"]
    want = {r[0]: list(r[1:]) for r in wanted(tkey, ["kd"], plain)}
    rows = []
    for key, vals in sorted(want.items()):
        mine = [k for k, g in enumerate(t["kd"]) if g == key]
        vals.insert(0, len({t["i2"][k] for k in mine} - {None}))
        vals.insert(4, len({t["j"][k] for k in mine} - {None}))
        rows.append((key,) + tuple(vals))
    assert ref.same_rows(got, rows)


@pytest.mark.gpu
def test_under_a_sort_and_limit_over_a_filter_and_as_a_join_input(gpu):
    tkey = (TILE + 1, 0.15)
    t = table(*tkey)
    aggs = A9
    ocols = [("kd", "Int32")] + [(agg_name(i, fn, arg), RESULT[fn](TYPES[arg] if arg else None)) for i, (fn, arg) in enumerate(aggs)]
    want = wanted(tkey, ["kd"], aggs)
    sort = {"execution_plan": "sort_exec", "input": whole_plan(["kd"], aggs), "expr": [{"expr": _c("kd", ocols), "options": {"descending": True, "nulls_first": False}}]}
    out = run(gpu, {"execution_plan": "global_limit_exec", "input": sort, "limit": 5}, [batches(t)])
    assert ref.same_rows(out_rows(out), sorted(want, reverse=True)[:5])
    # over a filter
    pred = _bin(_bin(_c("kd"), "Modulo", _lit("Int32", 3)), "Eq", _lit("Int32", 1))
    kept = {c: [v for v, k in zip(vals, t["kd"]) if k % 3 == 1] for c, vals in t.items()}
    out = run(gpu, whole_plan(["kd"], aggs, _filter(_scan(), pred)), [batches(t, 2)])
    assert ref.same_rows(ref.sort_rows(out_rows(out), 1), want_rows(kept, ["kd"], aggs))
    # as the input of a join
    lcols = [("want", "Int32")]
    left = {"execution_plan": "memory_exec", "schema": {"fields": [_field("want", "Int32")], "metadata": {}}, "projection": [0]}
    join = {"execution_plan": "hash_join_exec", "left": left, "right": whole_plan(["kd"], aggs), "join_type": "Inner", "mode": "CollectLeft",
            "on": [[_c("want", lcols), _c("kd", ocols)]], "schema": {"fields": [_field(n, ty) for n, ty in lcols + ocols], "metadata": {}}}
    asked = [103, 105, 105, 5000, 100]
    out = run(gpu, join, [[pa.record_batch([pa.array(asked, pa.int32())], names=["want"])], batches(t)])
    by_key = {r[0]: r for r in want}
    assert ref.same_rows(sorted(out_rows(out)), sorted((w,) + by_key[w] for w in asked if w in by_key))


@pytest.mark.gpu
def test_execute_twice_and_again_after_reset_with_other_rows(gpu):
    from flock_amd.runtime import ExecutionContext
    keys, aggs = ["ks", "kd"], A16_SUMS
    small, large = (TILE + 1, 0.15), (2 * TILE + 77, 0.15, 900, "hot")
    ctx = ExecutionContext([whole_plan(keys, aggs)], gpu=gpu)
    try:
        for tkey in (small, large, small):
            ctx.feed_data_sources([[batches(table(*tkey), 2)]])
            for _ in range(2):
                assert ref.same_rows(ref.sort_rows(out_rows(ctx.execute()[0]), len(keys)), wanted(tkey, keys, aggs))
            ctx.clean_data_sources()
    finally:
        ctx.close()


# ------------------------------------------------------------------ GPU 6: unchanged ground
@pytest.mark.gpu
def test_four_accumulators_keep_their_path_and_their_group_order(gpu):
    """A dense Int32 key under four integer accumulators without NULLs takes the direct-address table: its groups come out in KEY order, which is not the
    order of first appearance of this table (and so not the order of the path five accumulators take)."""
    tkey = (TILE + 1, 0.0)
    t = table(*tkey)
    aggs = [("count", None), ("sum", "i"), ("min", "l"), ("max", "j")]
    out = run(gpu, agg_node("Partial", ["kd"], aggs, _scan()), [batches(t)])
    rows = out_rows(out)
    assert [r[0] for r in rows] == sorted(set(t["kd"])) and [r[0] for r in rows] != list(dict.fromkeys(t["kd"]))
    assert rows == ref.sort_rows(ref.aggregate(t, ["kd"], aggs, TYPES), 1)
    five = out_rows(run(gpu, agg_node("Partial", ["kd"], aggs + [("max", "i")], _scan()), [batches(t)]))
    assert [r[0] for r in five] == list(dict.fromkeys(t["kd"]))       # five accumulators: order of first appearance


# ------------------------------------------------------------------ GPU 7: the fixture
@pytest.mark.gpu
def test_q17_auction_stats_over_generated_bids(gpu):
    """NEXMark q17 (auction statistics per auction and day) over a few thousand bids under NEXMark's skew (half of them on one auction), timestamps tied
    and spread over four days, prices over all three ranks -- whole and split at the repartition between Partial and FinalPartitioned."""
    from flock_amd import stages as S
    plan = json.load(open(os.path.join(PLANS, "q17_auction_stats.json")))
    r = np.random.default_rng(17)
    n = 6000
    day = 86_400_000
    auction = np.where(r.random(n) < 0.5, 1007, r.integers(1000, 1200, n)).astype(np.int32)
    bidder = np.where(r.random(n) < 0.75, 42, r.integers(0, 300, n)).astype(np.int32)
    price = np.floor(10 ** r.uniform(2, 7, n)).astype(np.int32)
    ts = 1_436_918_400_000 - 5_000 + (np.sort(r.integers(0, 4 * day, n)) // 60_000) * 60_000       # ties: whole minutes; the first day starts before midnight
    rb = pa.record_batch([pa.array(auction), pa.array(bidder), pa.array(price), pa.array(ts, pa.int64()).cast(pa.timestamp("ms"))],
                         names=["auction", "bidder", "price", "b_date_time"])
    p = price.tolist()
    t = {"auction": auction.tolist(), "day": (ts // day * day).tolist(), "price": p, "r1": [1 if v < 10000 else None for v in p],
         "r2": [1 if 10000 <= v < 1000000 else None for v in p], "r3": [1 if v >= 1000000 else None for v in p]}
    aggs = [("count", None), ("count", "r1"), ("count", "r2"), ("count", "r3"), ("min", "price"), ("max", "price"), ("avg", "price"), ("sum", "price")]
    want = ref.sort_rows(ref.aggregate(t, ["auction", "day"], aggs), 2)
    assert len(want) > 600 and all(sum(r[3:6]) == r[2] for r in want) and min(sum(r[k] for r in want) for k in (3, 4, 5)) > 500
    names = ["auction", "day", "total_bids", "rank1_bids", "rank2_bids", "rank3_bids", "MIN(price)", "MAX(price)", "AVG(price)", "SUM(price)"]
    for k in (1, 3):
        cuts = [n * j // k for j in range(k + 1)]
        out = run(gpu, plan, [[rb.slice(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]])
        assert ref.same_rows(ref.sort_rows(out_rows(out), 2), want)
        assert out[0].schema.names == names
    staged = S.StagedRun(gpu, S.build_query_dag(plan), instances=1, on_device=True)
    try:
        out = staged.run({"bid": rb})
    finally:
        staged.close()
    out = out if isinstance(out, list) else [out]
    assert ref.same_rows(ref.sort_rows(out_rows(out), 2), want)
