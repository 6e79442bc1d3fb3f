"""Aggregate window functions of window_agg_exec (relops.hpp window_aggregates, window.hip): COUNT / SUM / MIN / MAX / AVG over the default frame,
RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW, on an input that arrives sorted.  Row i gets the aggregate of its partition from the first row through
the last PEER of row i (equal ORDER BY values, NULL equal to NULL); without ORDER BY, the whole partition.  The reference is `reference_window` below,
checked against hand-worked tables; the oracle has ROW_NUMBER only."""
import json
import os

import numpy as np
import pyarrow as pa
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")

_TS = {"Timestamp": ["Millisecond", None]}
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string(), "ts": pa.timestamp("ms")}
# p / p2: PARTITION BY keys, o: ORDER BY key; the arguments: v Int64, i Int32, u UInt64, t Timestamp, f Float64; s Utf8
COLS = [("p", "Int32"), ("p2", "Int64"), ("o", "Int64"), ("v", "Int64"), ("i", "Int32"), ("u", "UInt64"), ("t", "ts"), ("f", "Float64"), ("s", "Utf8")]
TYPES = dict(COLS)
RESULT = {"count": lambda t: "UInt64", "avg": lambda t: "Float64", "sum": lambda t: "UInt64" if t == "UInt64" else "Int64",
          "min": lambda t: t, "max": lambda t: t}


def _dt(t):
    return _TS if t == "ts" else t


def _field(name, t, nullable=True):
    return {"data_type": _dt(t), "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


def _c(name, cols=COLS):
    return {"physical_expr": "column", "name": name, "index": [n for n, _ in cols].index(name)}


def _scan(cols=COLS):
    return {"execution_plan": "memory_exec", "schema": {"fields": [_field(n, t) for n, t in cols], "metadata": {}}, "projection": list(range(len(cols)))}


def _name(fn, arg):
    return "%s(%s)" % (fn.upper(), arg or "UInt8(1)")


def agg_entry(fn, arg, part, order=(), frame=None, cols=COLS, name=None):
    """One aggregate_window_expr entry: fn over column `arg` (None: COUNT(*)), PARTITION BY part, ORDER BY order (names, ascending)."""
    types = dict(cols)
    aggr = {"aggregate_expr": fn, "name": name or _name(fn, arg), "data_type": _dt(RESULT[fn](types[arg] if arg else None)), "nullable": True,
            "expr": _c(arg, cols) if arg else {"physical_expr": "literal", "value": {"UInt8": 1}}}
    e = {"window_expr": "aggregate_window_expr", "aggregate": aggr, "partition_by": [_c(p, cols) for p in part],
         "order_by": [{"expr": _c(o, cols), "options": {"descending": False, "nulls_first": False}} for o in order]}
    if frame is not None:
        e["window_frame"] = frame
    return e


def row_number_entry(part, cols=COLS):
    return {"window_expr": "built_in_window_expr", "fun": "RowNumber", "name": "rn", "partition_by": [_c(p, cols) for p in part], "order_by": []}


def window_plan(entries, cols=COLS):
    return {"execution_plan": "window_agg_exec", "input": _scan(cols), "window_expr": entries}


@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


# ------------------------------------------------------------------ the reference
def reference_window(cols, n, fn, arg, part, order=()):
    """Values and validity of one window column over `cols` (name -> (values ndarray, valid bool ndarray)) in input order.  Partitions are runs of equal
    PARTITION BY tuples, peer groups runs of equal (PARTITION BY, ORDER BY) tuples; NULL equals NULL."""
    def diff(names):
        d = np.zeros(n, bool)
        if n:
            d[0] = True
        for c in names:
            v, ok = cols[c]
            if n > 1:
                d[1:] |= (ok[1:] != ok[:-1]) | (ok[1:] & ok[:-1] & (v[1:] != v[:-1]))
        return d
    pstart = diff(part)
    gstart = diff(list(part) + list(order)) | pstart
    gid = np.cumsum(gstart) - 1
    gend_of_group = np.r_[np.nonzero(gstart)[0][1:] - 1, n - 1] if n else np.zeros(0, np.int64)
    ge = gend_of_group[gid] if n else gid       # the last row of every row's peer group
    starts = np.r_[np.nonzero(pstart)[0], n]
    if arg is None:
        vals, ok = np.zeros(n, np.int64), np.ones(n, bool)
    else:
        vals, ok = cols[arg]
    out = np.zeros(n, np.float64 if fn == "avg" else vals.dtype if fn in ("min", "max") else np.uint64 if (fn == "count" or vals.dtype == np.uint64) else np.int64)
    valid = np.ones(n, bool)
    for a, b in zip(starts[:-1], starts[1:]):
        seg_ok = ok[a:b]
        cnt = np.cumsum(seg_ok.astype(np.uint64))
        if fn == "count":
            scan, sv = cnt, np.ones(b - a, bool)
        elif fn in ("sum", "avg"):
            x = np.where(seg_ok, vals[a:b], 0).astype(np.uint64) if vals.dtype != np.uint64 else np.where(seg_ok, vals[a:b], 0)
            if vals.dtype == np.int32:
                x = np.where(seg_ok, vals[a:b].astype(np.int64), 0).view(np.uint64)
            s = np.cumsum(x, dtype=np.uint64)          # (wraps as two's complement)
            if fn == "sum":
                scan = s if vals.dtype == np.uint64 else s.view(np.int64)
            else:
                with np.errstate(invalid="ignore", divide="ignore"):
                    scan = s.view(np.int64).astype(np.float64) / cnt.astype(np.float64)
            sv = cnt > 0
        else:
            if vals.dtype == np.float64:
                ident = -np.inf if fn == "max" else np.inf
            else:
                info = np.iinfo(vals.dtype)
                ident = info.min if fn == "max" else info.max
            x = np.where(seg_ok, vals[a:b], ident).astype(vals.dtype)
            scan = (np.maximum if fn == "max" else np.minimum).accumulate(x)
            sv = cnt > 0
        idx = ge[a:b] - a
        out[a:b] = scan[idx]
        valid[a:b] = sv[idx]
    out[~valid] = 0
    return out, valid


def _hand_cols(rows, names):
    out = {}
    for k, name in enumerate(names):
        vs = [r[k] for r in rows]
        ok = np.array([x is not None for x in vs], bool)
        out[name] = (np.array([0 if x is None else x for x in vs], np.int64), ok)
    return out


def test_reference_against_hand_worked_tables():
    # (p, o, v): two partitions; peers (1, 10) x2 and (2, 5) x2; NULLs among the values and one NULL ORDER BY pair
    rows = [(1, 10, 4), (1, 10, None), (1, 20, 7), (1, None, 1), (1, None, 2), (2, 5, None), (2, 5, None), (2, 6, -3)]
    c = _hand_cols(rows, ["p", "o", "v"])
    n = len(rows)
    f = lambda fn, arg, order=("o",): [None if not ok else x.item() for x, ok in zip(*reference_window(c, n, fn, arg, ["p"], order))]
    assert f("count", None) == [2, 2, 3, 5, 5, 2, 2, 3]
    assert f("count", "v") == [1, 1, 2, 4, 4, 0, 0, 1]
    assert f("sum", "v") == [4, 4, 11, 14, 14, None, None, -3]
    assert f("max", "v") == [4, 4, 7, 7, 7, None, None, -3]
    assert f("min", "v") == [4, 4, 4, 1, 1, None, None, -3]
    assert f("avg", "v") == [4.0, 4.0, 5.5, 3.5, 3.5, None, None, -3.0]
    assert f("sum", "v", ()) == [14] * 5 + [-3] * 3           # no ORDER BY: the whole partition
    assert f("count", None, ()) == [5] * 5 + [3] * 3
    # NULL partition keys are one run; a wrapping Int64 SUM
    rows = [(None, 1, 2**62), (None, 1, 2**62), (None, 2, 2**62), (3, 1, 2**63 - 1), (3, 2, 1)]
    c = _hand_cols(rows, ["p", "o", "v"])
    assert [x.item() for x in reference_window(c, 5, "sum", "v", ["p"], ["o"])[0]] == [2**63 - 2**64, 2**63 - 2**64, -2**62, 2**63 - 1, -2**63]


# ------------------------------------------------------------------ CPU: parsing, refusals, stage split
FUNCS = [("count", None), ("count", "v"), ("sum", "v"), ("min", "i"), ("max", "u"), ("avg", "v"), ("max", "t"), ("min", "f")]


def test_every_function_parses_and_explains():
    from flock_amd.runtime import explain
    entries = [agg_entry(fn, arg, ["p"], ["o"]) for fn, arg in FUNCS] + [agg_entry("sum", "i", ["p", "p2"]), row_number_entry(["p"])]
    txt = explain(window_plan(entries))
    for s in ["COUNT(*) PARTITION BY p ORDER BY o", "COUNT(v) PARTITION BY p ORDER BY o", "SUM(v) PARTITION BY p ORDER BY o", "MIN(i) PARTITION BY p ORDER BY o",
              "MAX(u) PARTITION BY p ORDER BY o", "AVG(v) PARTITION BY p ORDER BY o", "MAX(t) PARTITION BY p", "MIN(f) PARTITION BY p",
              "SUM(i) PARTITION BY p p2, ROW_NUMBER PARTITION BY p)"]:
        assert s in txt, (s, txt)
    # result types: COUNT UInt64, SUM(Int32) Int64, MIN(Int32) Int32, AVG Float64, MAX(Timestamp) Timestamp
    for s in ["COUNT(UInt8(1)):UInt64", "SUM(v):Int64", "MIN(i):Int32", "MAX(u):UInt64", "AVG(v):Float64", "MAX(t):Timestamp(ms)", "SUM(i):Int64", "rn:UInt64"]:
        assert s in txt, (s, txt)
    # the default frame written out is taken too
    dflt = {"units": "Range", "start_bound": {"Preceding": None}, "end_bound": "CurrentRow"}
    assert "SUM(v) PARTITION BY p" in explain(window_plan([agg_entry("sum", "v", ["p"], ["o"], frame=dflt)]))
    assert "SUM(v) PARTITION BY p" in explain(window_plan([dict(agg_entry("sum", "v", ["p"], ["o"]), window_frame=None)]))


@pytest.mark.parametrize("entry,words", [
    (agg_entry("sum", "v", ["p"], ["o"], frame={"units": "Rows", "start_bound": {"Preceding": None}, "end_bound": "CurrentRow"}), "window frame Rows"),
    (agg_entry("max", "v", ["p"], ["o"], frame={"units": "Range", "start_bound": {"Preceding": 3}, "end_bound": "CurrentRow"}), "Preceding(3)"),
    (agg_entry("sum", "f", ["p"]), "sum needs an integer column"),
    (agg_entry("avg", "s", ["p"]), "avg needs an integer column"),
    (agg_entry("count", None, ["s"]), "PARTITION BY a Utf8 column"),
    (agg_entry("count", None, ["p", "p2", "o", "v", "i"]), "PARTITION BY more than four columns"),
    (agg_entry("count", None, ["p"], ["o", "v", "i", "u", "t"]), "ORDER BY more than four columns"),
])
def test_refusals_name_their_cause(entry, words):
    from flock_amd import FlockGpuError
    from flock_amd.runtime import explain
    with pytest.raises(FlockGpuError, match=words.replace("(", r"\(").replace(")", r"\)")):
        explain(window_plan([entry]))


def test_other_built_ins_stay_refused():
    from flock_amd import FlockGpuError
    from flock_amd.runtime import explain
    for fun in ["Rank", "DenseRank", "Lag", "Lead", "FirstValue"]:
        e = {"window_expr": "built_in_window_expr", "fun": fun, "name": fun, "partition_by": [_c("p")], "order_by": []}
        with pytest.raises(FlockGpuError) as err:
            explain(window_plan([e]))
        assert fun.lower() in str(err.value).lower() and "ROW_NUMBER" in str(err.value) and "MAX" in str(err.value)


def _q6_with(entry_fn):
    plan = json.load(open(os.path.join(PLANS, "q6.json")))
    node = plan
    while node.get("execution_plan") != "window_agg_exec":
        node = node["input"]
    node["window_expr"] = [entry_fn(node["window_expr"][0])]
    return plan


def _as_max_price(rn):
    """q6's outer ROW_NUMBER() (PARTITION BY seller ORDER BY b_date_time DESC) made MAX(b_date_time) over the same window"""
    return {"window_expr": "aggregate_window_expr", "partition_by": rn["partition_by"], "order_by": rn["order_by"],
            "aggregate": {"aggregate_expr": "max", "name": rn["name"], "data_type": _TS, "nullable": True, "expr": rn["order_by"][0]["expr"]}}


def test_stage_split_is_that_of_row_number():
    from flock_amd.runtime import explain
    from flock_amd.stages import build_query_dag
    rn = build_query_dag(_q6_with(lambda e: e))
    mx = build_query_dag(_q6_with(_as_max_price))
    assert len(rn) == len(mx) == 7

    def shape(o):
        if isinstance(o, dict):
            return {k: shape(v) for k, v in o.items() if k != "window_expr"}
        if isinstance(o, list):
            return [shape(x) for x in o]
        return o
    assert [shape(s.plan) for s in rn] == [shape(s.plan) for s in mx]
    assert "Window(MAX(b_date_time) PARTITION BY seller ORDER BY b_date_time DESC)" in explain(_q6_with(_as_max_price))


# ------------------------------------------------------------------ GPU: row for row against the reference
def _sorted_table(n, seed, part_sizes, peer_max, null_p, shape=""):
    """n rows already sorted by (p, o): partitions of the given sizes (cycled), peer groups of 1..peer_max rows; the arguments random, NULL with rate
    null_p.  shape "u_high": UInt64 values at or above 2^63; "wrap": Int64 values that overflow a sum."""
    r = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(part_sizes[len(sizes) % len(part_sizes)]) if len(part_sizes) else n)
    p = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)[:n]
    o = np.zeros(n, np.int64)
    if n:
        # peer groups: a new ORDER BY value every 1..peer_max rows (restarting per partition does not matter: the key only grows)
        steps = np.zeros(n, np.int64)
        pos = 0
        while pos < n:
            steps[pos] = 1
            pos += int(r.integers(1, peer_max + 1))
        o = np.cumsum(steps)
    cols = {"p": ((p * 7 - 3).astype(np.int32), np.ones(n, bool)), "p2": ((p // 3).astype(np.int64), np.ones(n, bool)), "o": (o, np.ones(n, bool)),
            "v": (r.integers(-10**9, 10**9, n).astype(np.int64), r.random(n) >= null_p),
            "i": (r.integers(-2**31, 2**31 - 1, n).astype(np.int32), r.random(n) >= null_p),
            "u": (r.integers(0, 2**63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1), r.random(n) >= null_p),
            "t": (1_436_918_400_000 + r.integers(0, 10**7, n).astype(np.int64), r.random(n) >= null_p),
            "f": (np.round(r.normal(0, 1000, n)), r.random(n) >= null_p),
            "s": (np.array([""] * n, dtype=object), np.ones(n, bool))}
    if shape == "u_high":
        cols["u"] = (np.uint64(2**63) + r.integers(0, 2**62, n, dtype=np.uint64), cols["u"][1])
    if shape == "wrap":
        cols["v"] = (np.int64(2**62) + r.integers(0, 2**61, n).astype(np.int64), cols["v"][1])
    if shape == "null_keys" and n:
        # NULL ORDER BY and PARTITION BY keys: runs of NULLs are equal to each other
        cols["o"] = (o, (o % 5) != 2)
        cols["p"] = (cols["p"][0], (p % 4) != 1)
    return cols


def _batches(cols, n, chunk):
    out = []
    for a in range(0, max(n, 1), chunk):
        arrs = []
        for name, t in COLS:
            v, ok = cols[name]
            v, ok = v[a:a + chunk], ok[a:a + chunk]
            if t == "Utf8":
                arrs.append(pa.array(list(v), pa.string()))
            elif t == "ts":
                arrs.append(pa.array(v, pa.int64(), mask=~ok).cast(pa.timestamp("ms")))
            else:
                arrs.append(pa.array(v, _PA[t], mask=~ok))
        out.append(pa.record_batch(arrs, names=[c for c, _ in COLS]))
    return out


def _column(out, name):
    arr = pa.concat_arrays([c for b in out for c in (b.column(b.schema.get_field_index(name)).chunks if hasattr(b.column(0), "chunks") else [b.column(b.schema.get_field_index(name))])])
    if pa.types.is_timestamp(arr.type):
        arr = arr.cast(pa.int64())
    ok = np.asarray(arr.is_valid())
    vals = arr.fill_null(0).to_numpy(zero_copy_only=False)
    return vals, ok


def _check(out, cols, n, fn, arg, part, order, name):
    got, gok = _column(out, name)
    want, wok = reference_window(cols, n, fn, arg, part, order)
    assert len(got) == n
    if fn == "count":
        assert gok.all()
    assert np.array_equal(gok, wok), (name, np.nonzero(gok != wok)[0][:10])
    assert np.array_equal(got[wok], want[wok].astype(got.dtype)), (name, np.nonzero(got[wok] != want[wok])[0][:10])


def _run(gpu, entries, cols, n, chunk=1 << 20, times=1):
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([window_plan(entries)], gpu=gpu)
    try:
        outs = [collect(ctx, [[_batches(cols, n, chunk)]])[0] for _ in range(times)]
    finally:
        ctx.close()
    return outs


ALL = [("count", None), ("count", "v"), ("sum", "v"), ("sum", "i"), ("min", "v"), ("max", "v"), ("min", "i"), ("max", "i"), ("avg", "v"), ("avg", "i"),
       ("min", "u"), ("max", "u"), ("min", "t"), ("max", "t"), ("sum", "u"), ("min", "f"), ("max", "f")]
# (rows, partition sizes, largest peer group, shape): 2048 rows make a tile
SHAPES = {"empty": (0, [1], 1, ""), "one_row": (1, [1], 1, ""), "own_partitions": (5000, [1], 1, ""),
          "straddle": (50_000, [3, 2047, 2049, 6000, 1, 4096 + 5, 700], 3000, ""), "peer_longer_than_tile": (20_000, [20_000], 5000, ""),
          "u_high": (9000, [100, 3000], 7, "u_high"), "wrap": (9000, [4500, 4500], 3, "wrap"), "null_keys": (10_000, [37, 2500], 9, "null_keys")}


def _entries(part, order):
    return [agg_entry(fn, arg, part, order, name="%s_%s_%s" % (fn, arg or "star", "o" if order else "p")) for fn, arg in ALL]


@pytest.mark.gpu
@pytest.mark.parametrize("null_p", [0.0, 0.2])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_function_row_for_row(gpu, shape, null_p):
    """Every function, with and without ORDER BY, in one node (two key groups, several passes each), against the reference row for row."""
    n, sizes, peer, kind = SHAPES[shape]
    cols = _sorted_table(n, 17 + n, sizes, peer, null_p, kind)
    entries = _entries(["p"], ["o"]) + _entries(["p"], [])
    out = _run(gpu, entries, cols, n, chunk=3001)[0]
    for e in entries:
        fn, arg, nm = e["aggregate"]["aggregate_expr"], e["aggregate"]["expr"].get("name"), e["aggregate"]["name"]
        _check(out, cols, n, fn, arg, ["p"], ["o"] if e["order_by"] else [], nm)
    if n:
        sch = out[0].schema
        assert sch.field("count_star_o").type == pa.uint64() and sch.field("sum_i_o").type == pa.int64() and sch.field("min_i_p").type == pa.int32()
        assert sch.field("avg_v_o").type == pa.float64() and sch.field("max_t_o").type == pa.timestamp("ms") and sch.field("max_u_p").type == pa.uint64()
        assert sch.names[len(entries):] == [c for c, _ in COLS]


@pytest.mark.gpu
@pytest.mark.parametrize("null_p", [0.0, 0.2])
def test_one_partition_of_ten_million_rows(gpu, null_p):
    """One partition over every tile, with and without ORDER BY (peer groups of up to 40 rows)."""
    n = 10_000_000
    cols = _sorted_table(n, 5, [n], 40, null_p)
    fns = [("count", None), ("sum", "v"), ("max", "v"), ("min", "i"), ("avg", "v")]
    entries = [agg_entry(fn, arg, ["p"], order, name="%s_%s_%d" % (fn, arg, len(order))) for order in (["o"], []) for fn, arg in fns]
    out = _run(gpu, entries, cols, n)[0]
    for e in entries:
        _check(out, cols, n, e["aggregate"]["aggregate_expr"], e["aggregate"]["expr"].get("name"), ["p"], ["o"] if e["order_by"] else [], e["aggregate"]["name"])


@pytest.mark.gpu
def test_row_number_with_three_aggregates_and_determinism(gpu):
    """ROW_NUMBER beside three aggregates of two key groups in one node; the output bytes are the same on every execute."""
    n = 30_000
    cols = _sorted_table(n, 9, [5, 3000, 2048, 777], 50, 0.2)
    entries = [row_number_entry(["p"]), agg_entry("max", "v", ["p"], ["o"], name="mx"), agg_entry("count", None, ["p"], name="cnt"),
               agg_entry("sum", "i", ["p"], ["o"], name="sm")]
    outs = _run(gpu, entries, cols, n, chunk=4096, times=3)
    out = outs[0]
    assert out[0].schema.names[:4] == ["rn", "mx", "cnt", "sm"]
    rn, ok = _column(out, "rn")
    p = cols["p"][0]
    first = np.r_[True, p[1:] != p[:-1]]
    assert ok.all() and np.array_equal(rn, np.arange(n) - np.maximum.accumulate(np.where(first, np.arange(n), 0)) + 1)
    _check(out, cols, n, "max", "v", ["p"], ["o"], "mx")
    _check(out, cols, n, "count", None, ["p"], [], "cnt")
    _check(out, cols, n, "sum", "i", ["p"], ["o"], "sm")
    for o in outs[1:]:
        for name in ["mx", "cnt", "sm"]:
            a = pa.concat_arrays([b.column(b.schema.get_field_index(name)) for b in out])
            b_ = pa.concat_arrays([b.column(b.schema.get_field_index(name)) for b in o])
            assert a.equals(b_)


# ------------------------------------------------------------------ through the plan ABI: NEXMark-shaped
BID = [("auction", "Int32"), ("price", "Int32"), ("b_date_time", "ts")]


def _bid_plan():
    """Each bid next to the best bid on its auction so far: MAX(price) OVER (PARTITION BY auction ORDER BY b_date_time), over the planner's
    Hash(auction) repartition and sort."""
    c = lambda nm: _c(nm, BID)
    rep = {"execution_plan": "repartition_exec", "input": _scan(BID), "partitioning": {"Hash": [[c("auction")], 4]}}
    srt = {"execution_plan": "sort_exec", "input": {"execution_plan": "coalesce_batches_exec", "input": rep, "target_batch_size": 4096},
           "expr": [{"expr": c("auction"), "options": {"descending": False, "nulls_first": False}},
                    {"expr": c("b_date_time"), "options": {"descending": False, "nulls_first": False}}]}
    e = agg_entry("max", "price", ["auction"], ["b_date_time"], cols=BID, name="best")
    return {"execution_plan": "window_agg_exec", "input": srt, "window_expr": [e]}


def _bids(n, seed):
    r = np.random.default_rng(seed)
    auction = r.integers(1000, 1400, n).astype(np.int32)
    price = r.integers(1, 10**6, n).astype(np.int32)
    ts = 1_436_918_400_000 + np.sort(r.integers(0, n // 4, n)).astype(np.int64)   # heavy ties
    rb = pa.record_batch([pa.array(auction), pa.array(price), pa.array(ts).cast(pa.timestamp("ms"))], names=[c for c, _ in BID])
    return auction, price, ts, rb


def _bid_reference(auction, price, ts):
    o = np.lexsort((ts, auction))
    a, p, t = auction[o].astype(np.int64), price[o].astype(np.int64), ts[o]
    cols = {"a": (a, np.ones(len(a), bool)), "t": (t, np.ones(len(a), bool)), "p": (p, np.ones(len(a), bool))}
    best, _ = reference_window(cols, len(a), "max", "p", ["a"], ["t"])
    return sorted(zip(a.tolist(), p.tolist(), t.tolist(), best.tolist()))


def _bid_rows(out):
    rows = []
    for b in out:
        d = {nm: b.column(b.schema.get_field_index(nm)) for nm in ["auction", "price", "b_date_time", "best"]}
        rows += list(zip(d["auction"].to_pylist(), d["price"].to_pylist(), d["b_date_time"].cast(pa.int64()).to_pylist(), d["best"].to_pylist()))
    return sorted(rows)


@pytest.mark.gpu
def test_running_max_bid_through_the_plan_abi_whole_and_staged(gpu):
    from flock_amd import stages as S
    from flock_amd.runtime import ExecutionContext, collect
    auction, price, ts, rb = _bids(60_000, 4)
    want = _bid_reference(auction, price, ts)
    ctx = ExecutionContext([_bid_plan()], gpu=gpu)
    for _ in range(2):
        out = collect(ctx, [[[rb.slice(a, 7000) for a in range(0, rb.num_rows, 7000)]]])[0]
        assert _bid_rows(out) == want
    assert out[0].schema.field("best").type == pa.int32()
    ctx.close()
    run = S.StagedRun(gpu, S.build_query_dag(_bid_plan()))
    out = run.run({"bid": rb})
    run.close()
    assert _bid_rows(out) == want
