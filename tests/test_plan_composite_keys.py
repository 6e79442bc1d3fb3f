"""GROUP BY, DISTINCT and inner joins on composite keys of mixed types (relops.hpp key_codes): the key shapes the one-key and pair paths refuse
-- three to eight columns, two columns that are not (Int32, Int32), NULLs in a multi-column key -- against the oracle
(oracle/generic_ops.py hash_aggregate_exec / hash_join_inner), which takes any number of keys."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pyarrow as pa
import pytest

from oracle import generic_ops as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")

_TS = {"Timestamp": ["Millisecond", None]}
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string(), "ts": pa.timestamp("ms")}
# the columns every table of this file carries: keys of every supported type, an integer and a float argument
COLS = [("i", "Int32"), ("i2", "Int32"), ("l", "Int64"), ("u", "UInt64"), ("t", "ts"), ("s", "Utf8"), ("s2", "Utf8"), ("l2", "Int64"), ("v", "Int64"),
        ("f", "Float64")]


def _dt(t):
    return _TS if t == "ts" else t


def _field(name, t, nullable=True):
    return {"data_type": _dt(t), "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


def _fields(cols=COLS):
    return [_field(n, t) for n, t in cols]


def _c(name, cols=COLS):
    return {"physical_expr": "column", "name": name, "index": [n for n, _ in cols].index(name)}


def _scan(cols=COLS):
    return {"execution_plan": "memory_exec", "schema": {"fields": _fields(cols), "metadata": {}}, "projection": list(range(len(cols)))}


def _group_plan(keys, aggs, cols=COLS):
    """Partial -> Hash([first key]) -> FinalPartitioned GROUP BY `keys`, aggs = [(fn, column or None, data_type)]."""
    def expr(fn, col, dt):
        arg = _c(col, cols) if col else {"physical_expr": "literal", "value": {"UInt8": 1}}
        return {"aggregate_expr": fn, "name": "%s(%s)" % (fn.upper(), col or "UInt8(1)"), "data_type": dt, "nullable": True, "expr": arg}
    ae = [expr(*a) for a in aggs]
    inschema = {"fields": _fields(cols), "metadata": {}}
    # the Partial's output schema (what the stage splitter gives the Final's leaf): keys, then the state columns of every aggregate
    types = dict(cols)
    states = []
    for e, (fn, _, dt) in zip(ae, aggs):
        states += [_field(e["name"] + "[count]", "UInt64"), _field(e["name"] + "[sum]", "Float64")] if fn == "avg" else [_field(e["name"] + "[%s]" % fn, dt)]
    pschema = {"fields": [_field(k, types[k]) for k in keys] + states, "metadata": {}}
    part = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [[_c(k, cols), k] for k in keys], "aggr_expr": ae, "input": _scan(cols),
            "input_schema": inschema, "schema": pschema}
    rep = {"execution_plan": "repartition_exec", "input": part, "partitioning": {"Hash": [[{"physical_expr": "column", "name": keys[0], "index": 0}], 4]}}
    return {"execution_plan": "hash_aggregate_exec", "mode": "FinalPartitioned",
            "group_expr": [[{"physical_expr": "column", "name": k, "index": i}, k] for i, k in enumerate(keys)],
            "aggr_expr": ae, "input": {"execution_plan": "coalesce_batches_exec", "input": rep, "target_batch_size": 4096},
            "input_schema": inschema, "schema": {"fields": [], "metadata": {}}}


def _join_plan(lcols, rcols, on):
    sc = lambda cols: {"execution_plan": "memory_exec", "schema": {"fields": _fields(cols), "metadata": {}}, "projection": list(range(len(cols)))}
    side = lambda cols, k: {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096,
                            "input": {"execution_plan": "repartition_exec", "input": sc(cols), "partitioning": {"Hash": [[_c(k, cols)], 4]}}}
    return {"execution_plan": "hash_join_exec", "left": side(lcols, on[0][0]), "right": side(rcols, on[0][1]), "join_type": "Inner", "mode": "Partitioned",
            "on": [[_c(a, lcols), _c(b, rcols)] for a, b in on], "schema": {"fields": _fields(lcols) + _fields(rcols), "metadata": {}}}


RCOLS = [(c + "_r", t) for c, t in COLS]     # (a join's right side: two leaves of one schema would read as one relation)
WORDS = ["", "a", "ab", "abc", "x" * 17, "y" * 17 + "z", "w" * 70, "w" * 69 + "v", "été", "key"]


def _table(n, seed, card, null_p=0.0, hot=0.0, nullable=("i", "i2", "l", "u", "t", "s", "s2", "l2")):
    """Columns of COLS; the key columns draw from `card` distinct tuples (0 = every row its own), one hot tuple takes a share `hot` of the rows,
    every key column of `nullable` is NULL with probability null_p.  v has no NULLs, f has some."""
    r = np.random.default_rng(seed)
    if card == 0:
        base = np.arange(n, dtype=np.int64)
    else:
        base = r.integers(0, card, n)
    base[r.random(n) < hot] = 7
    t = {"i": [int(x) for x in (base * 7919 % 100_003 - 50_000).astype(np.int32)],
         "i2": [int(x) for x in (base // 3 - 5).astype(np.int32)],
         "l": [int(x) for x in (base * 1_000_000_007 - 2**40)],
         "u": [int(x) for x in (base.astype(np.uint64) * np.uint64(2**61 + 3) + np.uint64(2**63))],
         "t": [1_436_918_400_000 + int(x) * 37 for x in base],
         "s": [WORDS[int(x) % len(WORDS)] + ("%d" % (x // len(WORDS)) if x >= len(WORDS) else "") for x in base],
         "s2": [WORDS[(int(x) * 3 + 1) % len(WORDS)] for x in base],
         "l2": [int(x) % 5 - 2 for x in base],
         "v": [int(x) for x in r.integers(-10**6, 10**6, n)],
         "f": [None if r.random() < 0.2 else float(x) for x in np.round(r.normal(0, 100, n))]}
    for c in nullable:
        if null_p > 0:
            m = r.random(n) < null_p
            t[c] = [None if m[i] else t[c][i] for i in range(n)]
    return t


def _batches(t, chunk, cols=COLS):
    n = len(t[cols[0][0]])
    out = []
    for a in range(0, max(n, 1), max(chunk, 1)):
        out.append(pa.record_batch([pa.array(t[c][a:a + chunk], _PA[ty]) for c, ty in cols], names=[c for c, _ in cols]))
    return out


def _pyrows(rb):
    cols = []
    for i in range(rb.num_columns):
        c = rb.column(i)
        if pa.types.is_timestamp(c.type):
            c = c.cast(pa.int64())
        cols.append(c.to_pylist())
    return list(zip(*cols))


def _oracle_rows(t, keys, aggs):
    want = g.hash_aggregate_exec(t, keys, [("%s(%s)" % (fn.upper(), col or "UInt8(1)"), fn, col) for fn, col, _ in aggs])
    return g.rows(want)


def _multiset(rows):
    return sorted(rows, key=repr)


# ------------------------------------------------------------------ CPU: parsing, recognition, stage split
def test_three_pair_join_parses():
    from flock_amd.runtime import explain
    plan = _join_plan(COLS, COLS, [("i", "i"), ("l", "l"), ("s", "s")])
    assert "Join" in explain(plan) or "join" in explain(plan).lower()
    nine = _join_plan(COLS, COLS, [(c, c) for c, _ in COLS[:8]] + [("v", "v")])
    from flock_amd.runtime import FlockGpuError
    with pytest.raises(FlockGpuError, match="8 key pairs"):
        explain(nine)


def test_q9_with_a_third_key_pair_is_generic():
    """q9's recogniser reads the join's two pairs; a third one must not be dropped silently: the plan runs on the generic operators."""
    from flock_amd import _ffi, build
    build.build()
    lib = _ffi.load()
    p = json.load(open(os.path.join(PLANS, "q9.json")))
    joins = []

    def walk(n):
        if isinstance(n, dict):
            if n.get("execution_plan") == "hash_join_exec" and len(n.get("on", [])) == 2:
                joins.append(n)
            for v in n.values():
                walk(v)
        elif isinstance(n, list):
            for v in n:
                walk(v)
    walk(p)
    assert len(joins) == 1
    t = json.dumps(p).encode()
    got = C.c_int(-1)
    assert lib.flockgpu_plan_recognise(t, len(t), C.byref(got)) == _ffi.OK and got.value == 9
    on = joins[0]["on"]
    on.append(copy.deepcopy(on[0]))        # auction = id a second time: the same rows, but a third pair
    t = json.dumps(p).encode()
    assert lib.flockgpu_plan_recognise(t, len(t), C.byref(got)) == _ffi.OK and got.value == 0


def test_three_pair_join_splits_like_a_one_pair_join():
    from flock_amd.stages import build_query_dag
    one = build_query_dag(_join_plan(COLS, COLS, [("i", "i")]))
    three = build_query_dag(_join_plan(COLS, COLS, [("i", "i"), ("t", "t"), ("s2", "s2")]))
    assert len(one) == len(three) == 3
    for a, b in zip(one, three):
        assert a.inputs == b.inputs and a.is_shuffling == b.is_shuffling and a.node == b.node
        assert json.dumps(a.plan).count("execution_plan") == json.dumps(b.plan).count("execution_plan")




# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


SHAPES = {
    "mix3": ["i", "s", "t"],
    "mix8": ["i", "l", "u", "t", "s", "s2", "i2", "l2"],
    "i32_ts": ["i", "t"],
    "utf8_utf8": ["s", "s2"],
    "i32_i32": ["i", "i2"],
}
AGGS = {
    "dense": [("count", None, "UInt64"), ("sum", "v", "Int64"), ("max", "v", "Int64")],          # no NULL arguments: the dense GROUP BY over the ids
    "hashed": [("count", "f", "UInt64"), ("min", "f", "Float64"), ("avg", "v", "Float64")],    # NULL / Float64 arguments: the hashed one
}


def _run_group(gpu, t, keys, aggs, chunk):
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([_group_plan(keys, aggs)], gpu=gpu)
    try:
        return collect(ctx, [[_batches(t, chunk)]])[0][0]
    finally:
        ctx.close()


# (rows, cardinality -- 0: every row its own key --, NULL rate, share of one hot key): each size with several cardinalities, 2049 is one row past a
# 2048-row tile
CASES = [(0, 1, 0.0, 0.0), (1, 1, 0.1, 0.0), (12, 1, 0.9, 0.0), (12, 6, 0.0, 0.0), (12, 0, 0.1, 0.0),
         (2049, 1, 0.0, 0.0), (2049, 1024, 0.1, 0.0), (2049, 0, 0.9, 0.0), (2049, 100, 0.0, 0.5),
         (40_000, 1, 0.1, 0.0), (40_000, 100, 0.0, 0.0), (40_000, 100, 0.9, 0.0), (40_000, 20_000, 0.1, 0.0), (40_000, 0, 0.0, 0.0), (40_000, 100, 0.1, 0.5)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("case", range(len(CASES)))
def test_group_by_composite_keys_row_for_row(gpu, shape, case):
    """Whole plan (Partial -> Hash -> FinalPartitioned): groups in order of first appearance, each group's keys those of its first row, equal to
    the oracle row for row -- NULL rates 0 / 0.1 / 0.9, cardinality 1 / ~100 / rows/2 / all unique, a hot key, 0 to 40000 rows."""
    keys = SHAPES[shape]
    n, card, null_p, hot = CASES[case]
    if shape == "i32_i32" and null_p == 0.0:
        null_p = 0.1          # (without NULLs this shape is the packed pair's)
    t = _table(n, 500 + case, card, null_p=null_p, hot=hot)
    for agg in sorted(AGGS):
        aggs = AGGS[agg]
        rb = _run_group(gpu, t, keys, aggs, max(1, n // 3))
        assert _pyrows(rb) == _oracle_rows(t, keys, aggs), (shape, case, agg)


@pytest.mark.gpu
def test_two_column_float64_keys_keep_their_messages(gpu):
    """Float64 key columns stay refused with the messages they had: the two-column GROUP BY's and DISTINCT's, the two-pair join's."""
    from flock_amd.runtime import ExecutionContext, collect
    t = _table(100, 1, 10)
    with pytest.raises(Exception, match=r"two-column GROUP BY other than \(Int32, Int32\) / \(Int32, Utf8\)"):
        _run_group(gpu, t, ["i", "f"], AGGS["dense"], 100)
    with pytest.raises(Exception, match=r"two-column GROUP BY other than \(Int32, Utf8\)"):
        _run_group(gpu, t, ["i", "f"], [], 100)
    t["f"] = [float(x) for x in range(100)]
    right = {c + "_r": v for c, v in t.items()}
    ctx = ExecutionContext([_join_plan(COLS, RCOLS, [("i", "i_r"), ("f", "f_r")])], gpu=gpu)
    with pytest.raises(Exception, match="a two-key join needs Int32 key columns"):
        collect(ctx, [[_batches(t, 100)], [_batches(right, 100, RCOLS)]])
    ctx.close()


@pytest.mark.gpu
def test_null_next_to_empty_string_and_long_strings(gpu):
    keys = ["s", "i"]
    t = {c: [] for c, _ in COLS}
    vals = ["", None, "", None, "a" * 65, "a" * 64 + "b", "a" * 65, "ab", "abc", "a", "", None]
    for j, s in enumerate(vals * 50):
        row = {"i": j % 2, "i2": 0, "l": 0, "u": 0, "t": 0, "s": s, "s2": "", "l2": 0, "v": j, "f": float(j)}
        for c, _ in COLS:
            t[c].append(row[c])
    aggs = AGGS["dense"]
    rb = _run_group(gpu, t, keys, aggs, 100)
    got = _pyrows(rb)
    assert got == _oracle_rows(t, keys, aggs)
    assert {r[0] for r in got} >= {"", None}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [12, 5_000, 1_000_000])
def test_distinct_int32_utf8_with_nulls(gpu, n):
    keys = ["i", "s"]
    t = _table(n, 11, max(1, n // 4), null_p=0.1, nullable=("i", "s"))
    rb = _run_group(gpu, t, keys, [], max(1, n // 2))
    assert _pyrows(rb) == _oracle_rows(t, keys, [])


@pytest.mark.gpu
def test_group_by_more_than_eight_columns_is_refused_with_its_limit(gpu):
    keys = [c for c, _ in COLS[:8]] + ["v"]
    t = _table(100, 1, 10)
    with pytest.raises(Exception, match="more than 8 columns"):
        _run_group(gpu, t, keys, AGGS["dense"], 100)


@pytest.mark.gpu
def test_float64_group_key_stays_refused(gpu):
    t = _table(100, 1, 10)
    with pytest.raises(Exception, match="Float64"):
        _run_group(gpu, t, ["i", "s", "f"], AGGS["dense"], 100)


@pytest.mark.gpu
def test_group_by_million_rows_three_keys(gpu):
    keys = ["i", "t", "s"]
    t = _table(1_000_000, 3, 300_000, null_p=0.1)
    aggs = AGGS["dense"]
    rb = _run_group(gpu, t, keys, aggs, 250_000)
    assert _pyrows(rb) == _oracle_rows(t, keys, aggs)


@pytest.mark.gpu
def test_same_output_bytes_on_every_execute(gpu):
    from flock_amd.runtime import ExecutionContext, collect
    keys = ["s", "l", "i2"]
    t = _table(30_000, 21, 3_000, null_p=0.1)
    ctx = ExecutionContext([_group_plan(keys, AGGS["hashed"])], gpu=gpu)
    outs = [collect(ctx, [[_batches(t, 10_000)]])[0][0] for _ in range(3)]
    ctx.close()
    assert outs[0].num_rows > 0 and outs[0].equals(outs[1]) and outs[1].equals(outs[2])


@pytest.mark.gpu
@pytest.mark.parametrize("agg", sorted(AGGS))
def test_stage_by_stage_equals_the_oracle_as_a_multiset(gpu, agg):
    """The plan split at its hash repartition (build_query_dag): the Partial stage runs execute_partitioned, the FinalPartitioned stage groups
    every partition's states again -- on the composite ids, with the states' own key columns."""
    from flock_amd.runtime import ExecutionContext
    from flock_amd.stages import build_query_dag
    keys = ["i", "s", "t"]
    aggs = AGGS[agg]
    t = _table(20_000, 31, 2_000, null_p=0.1)
    stages = build_query_dag(_group_plan(keys, aggs))
    assert len(stages) == 2 and stages[0].is_shuffling
    c0 = ExecutionContext([stages[0].plan], gpu=gpu)
    c0.feed_data_sources([[_batches(t, 7_000)]])
    parts = c0.execute_partitioned()[0]
    c0.clean_data_sources()
    c0.close()
    batches = [b for p in parts for b in p if b.num_rows > 0]
    c1 = ExecutionContext([stages[1].plan], gpu=gpu)
    c1.feed_data_sources([[batches]])
    out = c1.execute()[0][0]
    c1.close()
    want = _oracle_rows(t, keys, aggs)
    assert out.num_rows == len(want)
    assert _multiset(_pyrows(out)) == _multiset(want)


def _join_tables(nl, nr, seed, null_p):
    r = np.random.default_rng(seed)
    card = max(2, min(nl, nr) // 3) if min(nl, nr) > 0 else 2
    left = _table(nl, seed, card, null_p=null_p)
    right = _table(nr, seed + 1, card * 2, null_p=null_p)
    right["v"] = [int(x) for x in r.integers(0, 9, nr)]
    return left, right


JOINS = {
    "three": [("i", "i"), ("l", "l"), ("s", "s")],
    "mixed": [("i", "l"), ("t", "t")],           # Int32 = Int64 by value, Timestamp = Timestamp
    "utf8": [("s", "s"), ("s2", "s2")],
    "eight": [("i", "i"), ("i2", "i2"), ("l", "l"), ("u", "u"), ("t", "t"), ("s", "s"), ("s2", "s2"), ("l2", "l2")],
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(JOINS))
@pytest.mark.parametrize("nl,nr,null_p", [(3_000, 800, 0.0), (700, 5_000, 0.1), (0, 500, 0.0), (400, 0, 0.1), (1, 1, 0.0), (20_000, 20_000, 0.1)])
def test_join_on_composite_keys(gpu, shape, nl, nr, null_p):
    """Every (left, right) pair with equal keys, as a multiset: NULL keys on both sides (match nothing), duplicate keys on both sides, empty sides."""
    from flock_amd.runtime import ExecutionContext, collect
    on = [(a, b + "_r") for a, b in JOINS[shape]]
    left, right = _join_tables(nl, nr, nl * 7 + nr, null_p)
    if shape == "mixed":      # make Int32 i meet Int64 l by value: l carries the values of i on the other side
        left["i"] = [None if x is None else x % 1000 for x in left["i"]]
        right["l"] = [None if x is None else x % 1000 for x in right["i"]]
    right = {c + "_r": v for c, v in right.items()}
    ctx = ExecutionContext([_join_plan(COLS, RCOLS, on)], gpu=gpu)
    out = collect(ctx, [[_batches(left, 5_000)], [_batches(right, 5_000, RCOLS)]])[0][0]
    ctx.close()
    want = g.rows(g.hash_join_inner(left, right, on))
    got = _pyrows(out)
    assert len(got) == len(want), (shape, nl, nr, null_p)
    assert _multiset(got) == _multiset(want)
    if nl and nr:
        assert len(want) > 0


_FILTERED_JOINS = dict(JOINS, i32_pair=[("i", "i"), ("i2", "i2")], one=[("i", "i")])   # + the packed Int32 pair, + one pair


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(_FILTERED_JOINS))
@pytest.mark.parametrize("nl,nr,null_p", [(700, 500, 0.1), (20_000, 12_000, 0.1)])
def test_join_on_composite_keys_under_filters(gpu, shape, nl, nr, null_p):
    """An inner join whose two inputs are filters: both sides arrive as row lists, and every key column -- the second and later pairs too -- is read
    through them.  (700, 500) stays inside the one-workgroup join; at (20000, 12000) the smaller side has more than 4096 rows and leaves it."""
    from flock_amd.runtime import ExecutionContext, collect
    on = [(a, b + "_r") for a, b in _FILTERED_JOINS[shape]]
    left, right = _join_tables(nl, nr, nl * 7 + nr, null_p)
    if shape == "mixed":      # (as in test_join_on_composite_keys: Int32 i meets Int64 l by value)
        left["i"] = [None if x is None else x % 1000 for x in left["i"]]
        right["l"] = [None if x is None else x % 1000 for x in right["i"]]
    right = {c + "_r": v for c, v in right.items()}
    lit = lambda v: {"physical_expr": "literal", "value": {"Int64": v}}
    plan = _join_plan(COLS, RCOLS, on)
    plan["left"] = {"execution_plan": "filter_exec", "input": plan["left"],
                    "predicate": {"physical_expr": "binary_expr", "left": _c("v"), "op": "Gt", "right": lit(-500_000)}}
    plan["right"] = {"execution_plan": "filter_exec", "input": plan["right"],
                     "predicate": {"physical_expr": "binary_expr", "left": _c("v_r", RCOLS), "op": "GtEq", "right": lit(3)}}
    ctx = ExecutionContext([plan], gpu=gpu)
    out = collect(ctx, [[_batches(left, 5_000)], [_batches(right, 5_000, RCOLS)]])[0][0]
    ctx.close()
    want = g.rows(g.hash_join_inner(g.filter_exec(left, lambda r: r["v"] > -500_000), g.filter_exec(right, lambda r: r["v_r"] >= 3), on))
    got = _pyrows(out)
    assert len(want) > 0
    assert len(got) == len(want), (shape, nl, nr, null_p)
    assert _multiset(got) == _multiset(want)


@pytest.mark.gpu
@pytest.mark.parametrize("nr", [50, 2_000])
def test_join_on_a_computed_key_that_holds_nulls(gpu, nr):
    """A grouped MIN over nothing but NULLs is NULL; joined on with two more key pairs, its rows match nothing.  The NULLs reach the composite
    ids (a leaf's NULL join keys are dropped at feed, a computed column's are not): with 50 right rows the groups probe (a NULL probe key),
    with 2000 the groups are the build side (NULL build tuples)."""
    from flock_amd.runtime import ExecutionContext, collect
    t = _table(3_000, 77, 300)
    t["v"] = [None if (t["i2"][k] % 3 == 0) else t["v"][k] for k in range(3_000)]          # every group with i2 % 3 == 0: MIN(v) is NULL
    groups = g.hash_aggregate_exec(t, ["i", "s2"], [("MIN(v)[min]", "min", "v")])
    assert None in groups["MIN(v)[min]"]
    r = np.random.default_rng(nr)
    pick = r.integers(0, len(groups["i"]), nr)
    right = {c: [] for c, _ in RCOLS}
    for j, q in enumerate(pick):
        for c, _ in COLS:
            right[c + "_r"].append(t[c][j % 3_000])
        right["i_r"][-1], right["s2_r"][-1] = groups["i"][q], groups["s2"][q]
        m = groups["MIN(v)[min]"][q]
        right["v_r"][-1] = m if m is not None and j % 4 else int(r.integers(-10**6, 10**6))   # (a NULL MIN gets a value: it must still not match)
    ae = [{"aggregate_expr": "min", "name": "MIN(v)", "data_type": "Int64", "nullable": True, "expr": _c("v")}]
    left = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [[_c("i"), "i"], [_c("s2"), "s2"]], "aggr_expr": ae, "input": _scan(),
            "input_schema": {"fields": _fields(), "metadata": {}}, "schema": {"fields": [], "metadata": {}}}
    lf = [("i", "Int32"), ("s2", "Utf8"), ("MIN(v)[min]", "Int64")]
    plan = {"execution_plan": "hash_join_exec", "left": left, "right": _scan(RCOLS), "join_type": "Inner", "mode": "CollectLeft",
            "on": [[_c("i", lf), _c("i_r", RCOLS)], [_c("s2", lf), _c("s2_r", RCOLS)], [_c("MIN(v)[min]", lf), _c("v_r", RCOLS)]],
            "schema": {"fields": _fields(lf) + _fields(RCOLS), "metadata": {}}}
    ctx = ExecutionContext([plan], gpu=gpu)
    out = collect(ctx, [[_batches(t, 1_000)], [_batches(right, 1_000, RCOLS)]])[0][0]
    ctx.close()
    want = g.rows(g.hash_join_inner(groups, right, [("i", "i_r"), ("s2", "s2_r"), ("MIN(v)[min]", "v_r")]))
    assert len(want) > 0 and _multiset(_pyrows(out)) == _multiset(want)


@pytest.mark.gpu
def test_two_joins_that_differ_in_their_third_pair(gpu):
    """One plan holding two joins that differ only in their third key pair: two different sub-results (the node signature names every pair)."""
    from flock_amd.runtime import ExecutionContext, collect
    cols = [("i", "Int32"), ("l", "Int64"), ("s", "Utf8"), ("s2", "Utf8"), ("v", "Int64")]
    bcols = [(c + "_r", t) for c, t in cols]
    n = 600

    def side(seed, sfx):
        q = np.random.default_rng(seed)
        t = {"i": [int(x) for x in q.integers(0, 20, n)], "l": [int(x) for x in q.integers(0, 3, n)], "s": ["s%d" % x for x in q.integers(0, 3, n)],
             "s2": ["t%d" % x for x in q.integers(0, 2, n)], "v": list(range(n))}
        return {c + sfx: v for c, v in t.items()}
    a, b = side(1, ""), side(2, "_r")
    p3 = [("i", "i_r"), ("l", "l_r"), ("s", "s_r")]
    p4 = [("i", "i_r"), ("l", "l_r"), ("s2", "s2_r")]
    j3, j4 = _join_plan(cols, bcols, p3), _join_plan(cols, bcols, p4)
    width = len(cols) + len(bcols)
    jf = _fields(cols) + _fields(bcols)
    top = {"execution_plan": "hash_join_exec", "left": j3, "right": j4, "join_type": "Inner", "mode": "CollectLeft",
           "on": [[{"physical_expr": "column", "name": "v", "index": 4}, {"physical_expr": "column", "name": "v", "index": 4}]],
           "schema": {"fields": jf + jf, "metadata": {}}}
    ctx = ExecutionContext([top], gpu=gpu)
    out = collect(ctx, [[_batches(a, n, cols)], [_batches(b, n, bcols)], [_batches(a, n, cols)], [_batches(b, n, bcols)]])[0][0]
    ctx.close()
    r3, r4 = g.rows(g.hash_join_inner(a, b, p3)), g.rows(g.hash_join_inner(a, b, p4))
    assert _multiset(r3) != _multiset(r4)
    want = [x + y for x in r3 for y in r4 if x[4] == y[4]]
    got = _pyrows(out)
    assert out.num_columns == 2 * width and len(want) > 0 and _multiset(got) == _multiset(want)


@pytest.mark.gpu
def test_three_key_group_by_over_92_million_bids(gpu):
    """GROUP BY auction, bidder % 97, price % 13 over 9.2e7 bid-shaped rows: the row count and the sums of COUNT(*) and SUM(price) equal numpy's."""
    from flock_amd.runtime import ExecutionContext, collect
    r = np.random.default_rng(92)
    n = 92_000_000
    auction = r.integers(1000, 1000 + 60_000, n).astype(np.int32)
    bidder = (r.integers(0, 97, n)).astype(np.int32)
    price = (r.integers(0, 13, n)).astype(np.int32)
    cols = [("auction", "Int32"), ("bidder", "Int32"), ("price", "Int32")]
    fields = [_field(c, t, False) for c, t in cols]
    scan_ = {"execution_plan": "memory_exec", "schema": {"fields": fields, "metadata": {}}, "projection": [0, 1, 2]}
    cc = lambda name: {"physical_expr": "column", "name": name, "index": [c for c, _ in cols].index(name)}
    ae = [{"aggregate_expr": "count", "name": "COUNT(UInt8(1))", "data_type": "UInt64", "nullable": True, "expr": {"physical_expr": "literal", "value": {"UInt8": 1}}},
          {"aggregate_expr": "sum", "name": "SUM(price)", "data_type": "Int64", "nullable": True, "expr": cc("price")}]
    plan = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [[cc(c), c] for c, _ in cols], "aggr_expr": ae, "input": scan_,
            "input_schema": {"fields": fields, "metadata": {}}, "schema": {"fields": [], "metadata": {}}}
    rb = [pa.record_batch([pa.array(auction), pa.array(bidder), pa.array(price)], names=[c for c, _ in cols])]
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        out = collect(ctx, [[rb]])[0][0]
    finally:
        ctx.close()
    packed = (auction.astype(np.int64) << 16) | (bidder.astype(np.int64) << 8) | price.astype(np.int64)
    n_groups = len(np.unique(packed))
    assert out.num_rows == n_groups
    assert int(out.column(3).to_numpy().astype(np.int64).sum()) == n
    assert int(out.column(4).to_numpy().sum()) == int(price.astype(np.int64).sum())
    assert [out.column(c)[0].as_py() for c in range(3)] == [int(auction[0]), int(bidder[0]), int(price[0])]     # groups in order of first appearance
