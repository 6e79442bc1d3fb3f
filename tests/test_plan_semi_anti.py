"""HashJoinExec join_type Semi / Anti (relops.hpp A-S1..6): the rows of the LEFT input that have / lack a partner on the right, in left order,
with the left input's schema -- against the plain-Python reference of tests/semi_anti_ref.py, row for row."""
import ctypes as C
import json
import os

import numpy as np
import pyarrow as pa
import pytest

from semi_anti_ref import semi_anti_rows, semi_anti_table, table_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")

_TS = {"Timestamp": ["Millisecond", None]}
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string(), "ts": pa.timestamp("ms")}
# the columns every generated table carries: keys of every supported type, Utf8 payload, an integer and a float column (f holds NULLs)
COLS = [("i", "Int32"), ("i2", "Int32"), ("l", "Int64"), ("u", "UInt64"), ("t", "ts"), ("s", "Utf8"), ("s2", "Utf8"), ("l2", "Int64"), ("v", "Int64"),
        ("f", "Float64")]
RCOLS = [(c + "_r", t) for c, t in COLS]     # (the right side: two leaves of one schema would read as one relation)
NAMES = [c for c, _ in COLS]
WORDS = ["", "a", "ab", "abc", "x" * 17, "y" * 17 + "z", "w" * 70, "w" * 69 + "v", "été", "key"]
TILE = 8192                                   # rows of one flag tile of the probe


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


def _coalesce(inp):
    return {"execution_plan": "coalesce_batches_exec", "input": inp, "target_batch_size": 4096}


def _hash(inp, key, cols, parts=4):
    return {"execution_plan": "repartition_exec", "input": inp, "partitioning": {"Hash": [[_c(key, cols)], parts]}}


def _filter(inp, pred):
    return {"execution_plan": "filter_exec", "predicate": pred, "input": inp}


def _ge0(name, cols):
    return {"physical_expr": "binary_expr", "left": _c(name, cols), "op": "GtEq", "right": {"physical_expr": "literal", "value": {"Int64": 0}}}


def _join(jt, left, right, lcols, rcols, on, mode="Partitioned", out=None):
    """hash_join_exec over two finished inputs; out = the node's schema columns (default: left only for Semi / Anti, both sides for Inner)."""
    if out is None:
        out = list(lcols) + (list(rcols) if jt == "Inner" else [])
    return {"execution_plan": "hash_join_exec", "left": left, "right": right, "join_type": jt, "mode": mode,
            "on": [[_c(a, lcols), _c(b, rcols)] for a, b in on], "schema": {"fields": _fields(out), "metadata": {}}}


def _semi_plan(jt, on, lcols=COLS, rcols=RCOLS, mode="Partitioned", parts=4, lpred=None, rpred=None):
    def side(cols, key, pred):
        inp = _scan(cols)
        if pred is not None:
            inp = _coalesce(_filter(inp, pred))
        return _coalesce(_hash(inp, key, cols, parts))
    return _join(jt, side(lcols, on[0][0], lpred), side(rcols, on[0][1], rpred), lcols, rcols, on, mode)


def _table(n, seed, card, null_p=0.0, hot=0.0, nullable=("i", "i2", "l", "u", "t", "s", "s2", "l2")):
    """Columns of COLS; the key columns draw from `card` distinct tuples (0 = every row its own), one hot tuple takes a share `hot` of the rows,
    every key column of `nullable` is NULL with probability null_p.  v has no NULLs, f has some."""
    r = np.random.default_rng(seed)
    base = np.arange(n, dtype=np.int64) if card == 0 else r.integers(0, card, n)
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


def _pair(nl, nr, seed, null_l=0.0, null_r=0.0, hot=0.0):
    """A left and a right table whose keys overlap in part: the right side draws from half the left side's key tuples."""
    k = max(1, min(max(nl, 1), max(nr, 1)) // 3)
    left = _table(nl, seed, 2 * k, null_p=null_l)
    right = _table(nr, seed + 1, k, null_p=null_r, hot=hot)
    return left, {c + "_r": v for c, v in right.items()}


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
    return list(zip(*cols)) if cols else []


def _multiset(rows):
    return sorted(rows, key=repr)


def _want(left, right, on, anti, names=NAMES):
    return table_rows(semi_anti_table(left, right, on, anti), names)


# ------------------------------------------------------------------ CPU: the reference itself
def test_reference_on_hand_worked_rows():
    left = {"k": [1, None, 2, 2, 3, None], "p": ["a", "b", "c", "d", "e", "f"]}
    right = {"q": [2, 2, None, 5, 2]}
    assert semi_anti_rows(left, right, [("k", "q")], False) == [2, 3]               # both rows with key 2, each once (A-S3); NULLs dropped
    assert semi_anti_rows(left, right, [("k", "q")], True) == [0, 1, 4, 5]          # NULL-keyed left rows are KEPT by Anti (A-S4)
    assert semi_anti_rows(left, {"q": []}, [("k", "q")], False) == []               # empty right
    assert semi_anti_rows(left, {"q": []}, [("k", "q")], True) == [0, 1, 2, 3, 4, 5]
    assert semi_anti_rows({"k": [], "p": []}, right, [("k", "q")], True) == []      # empty left
    assert semi_anti_rows(left, {"q": [None, None]}, [("k", "q")], False) == []     # a NULL right key matches nothing, not even a NULL
    two_l = {"a": [1, 1, None, 2], "b": ["x", None, "x", "y"]}
    two_r = {"c": [1, 2, 2, None], "d": ["x", "y", None, "x"]}
    assert semi_anti_rows(two_l, two_r, [("a", "c"), ("b", "d")], False) == [0, 3]
    assert semi_anti_rows(two_l, two_r, [("a", "c"), ("b", "d")], True) == [1, 2]
    assert table_rows(semi_anti_table(left, right, [("k", "q")], False), ["k", "p"]) == [(2, "c"), (2, "d")]


@pytest.mark.parametrize("seed", range(6))
def test_reference_against_pyarrow(seed):
    """Acero's left semi / left anti on random tables with NULLs on both sides, one and two key columns: the same rows as multisets (Acero gives no order)."""
    r = np.random.default_rng(seed)
    nl, nr = int(r.integers(0, 400)), int(r.integers(0, 300))

    def col(n, hi, p):
        return [None if r.random() < p else int(x) for x in r.integers(0, hi, n)]
    left = {"a": col(nl, 40, 0.15), "b": [None if r.random() < 0.1 else WORDS[int(x)] for x in r.integers(0, 4, nl)], "row": list(range(nl))}
    right = {"c": col(nr, 30, 0.15), "d": [None if r.random() < 0.1 else WORDS[int(x)] for x in r.integers(0, 4, nr)]}
    lt = pa.table({"a": pa.array(left["a"], pa.int64()), "b": pa.array(left["b"], pa.string()), "row": pa.array(left["row"], pa.int64())})
    rt = pa.table({"c": pa.array(right["c"], pa.int64()), "d": pa.array(right["d"], pa.string())})
    for on in ([("a", "c")], [("a", "c"), ("b", "d")]):
        for anti in (False, True):
            got = lt.join(rt, keys=[a for a, _ in on], right_keys=[b for _, b in on], join_type="left anti" if anti else "left semi")
            assert sorted(got.column("row").to_pylist()) == semi_anti_rows(left, right, on, anti), (seed, on, anti)


# ------------------------------------------------------------------ CPU: parsing, recognition, stage split
def test_explain_names_the_nodes_and_the_left_only_schema():
    from flock_amd.runtime import explain
    for jt in ("Semi", "Anti"):
        text = explain(_semi_plan(jt, [("i", "i_r")]))
        lines = text.splitlines()
        assert lines[0].startswith(jt + "Join [") and "Join" not in lines[0].replace(jt + "Join", ""), text
        assert "i:Int32" in lines[0] and "f:Float64" in lines[0] and "_r:" not in lines[0], text          # the left input's columns, none of the right's
        assert lines[0].count(":") == len(COLS), text
    for name, jt in (("semi_join", "Semi"), ("anti_join", "Anti")):      # the golden join of the fixtures (bare key names, Utf8 keys) as Semi / Anti
        lines = explain(open(os.path.join(PLANS, name + ".json")).read()).splitlines()
        assert lines[0] == "Project [a:Utf8, b:Int32]" and lines[1].strip().startswith(jt + "Join [a:Utf8, b:Int32]") and lines[-1].endswith("reads [c]"), lines
    inner = explain(_join("Inner", _scan(COLS), _scan(RCOLS), COLS, RCOLS, [("i", "i_r")]))
    assert inner.splitlines()[0].startswith("Join [") and "i_r:Int32" in inner.splitlines()[0]


def test_right_leaf_uploads_only_its_key_columns():
    """mark_required: nothing above a Semi / Anti join reads a right column, so the right leaf needs its keys and nothing else (an Inner join's
    right leaf needs every column the output shows); the left leaf needs what the output shows."""
    from flock_amd.runtime import explain
    for jt, on in (("Semi", [("i", "i_r")]), ("Anti", [("s", "s_r"), ("l", "l_r")])):
        scans = [ln.strip() for ln in explain(_semi_plan(jt, on)).splitlines() if ln.strip().startswith("Scan")]
        assert len(scans) == 2, scans
        assert "reads" not in scans[0]
        assert scans[1].endswith("reads [" + ", ".join(b for _, b in sorted(on, key=lambda p: NAMES.index(p[0]))) + "]"), scans[1]
    # a projection on top that names two left columns: the right leaf still reads its key alone
    top = {"execution_plan": "projection_exec", "expr": [[_c("v"), "v"], [_c("s2"), "s2"]], "input": _semi_plan("Anti", [("t", "t_r")]),
           "schema": {"fields": [_field("v", "Int64"), _field("s2", "Utf8")], "metadata": {}}}
    text = explain(top)
    assert text.splitlines()[0].startswith("Project [v:Int64, s2:Utf8]") and "reads [t_r]" in text


def _refused(plan, *words):
    from flock_amd import _ffi
    from flock_amd.runtime import FlockGpuError, explain
    with pytest.raises(FlockGpuError) as e:
        explain(plan)
    assert e.value.code == _ffi.ERR_UNSUPPORTED, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals_by_name():
    on = [("i", "i_r")]
    for jt in ("Semi", "Anti"):
        both = _semi_plan(jt, on)
        both["schema"] = {"fields": _fields(COLS) + _fields(RCOLS), "metadata": {}}      # right columns carried along: another operator's schema
        _refused(both, jt, "schema", "left")
        wrong = _semi_plan(jt, on)
        wrong["schema"]["fields"][0]["data_type"] = "Int64"                               # same count, another type
        _refused(wrong, jt, "schema")
        _refused(_semi_plan(jt, [("f", "f_r")]), "join keys must be integer columns of one signedness, or two Utf8 columns")
        _refused(_semi_plan(jt, [("i", "i_r"), ("f", "f_r")]), "join keys must be integer columns of one signedness, or two Utf8 columns")
        _refused(_semi_plan(jt, [("s", "i_r")]), "join keys must be integer columns of one signedness, or two Utf8 columns")
        _refused(_semi_plan(jt, [("u", "l_r")]), "join keys must be integer columns of one signedness, or two Utf8 columns")
        _refused(_semi_plan(jt, [(c, c + "_r") for c in NAMES[:8]] + [("v", "v_r")]), "8 key pairs")
    for jt in ("Left", "Right", "Full"):
        p = _semi_plan("Semi", on)
        p["join_type"] = jt
        _refused(p, jt, "Inner", "Semi", "Anti")


def _q3_semi(jt="Semi"):
    """q3's plan with the join turned into a Semi join: the auctions of category 10 whose seller lives in or / id / ca -- left columns only."""
    p = json.load(open(os.path.join(PLANS, "q3.json")))
    j = p["input"]["input"]
    assert j["execution_plan"] == "hash_join_exec"
    j["join_type"] = jt
    j["schema"]["fields"] = j["schema"]["fields"][:3]
    p["expr"] = [[{"physical_expr": "column", "name": "a_id", "index": 0}, "a_id"], [{"physical_expr": "column", "name": "seller", "index": 1}, "seller"]]
    p["schema"]["fields"] = [j["schema"]["fields"][0], j["schema"]["fields"][1]]
    return p


def test_q3_look_alike_with_semi_is_not_fused():
    from flock_amd import _ffi, build
    from flock_amd.runtime import explain
    build.build()
    lib = _ffi.load()
    got = C.c_int(-1)
    t = open(os.path.join(PLANS, "q3.json")).read().encode()
    assert lib.flockgpu_plan_recognise(t, len(t), C.byref(got)) == _ffi.OK and got.value == 3
    for jt in ("Semi", "Anti"):
        p = _q3_semi(jt)
        t = json.dumps(p).encode()
        assert lib.flockgpu_plan_recognise(t, len(t), C.byref(got)) == _ffi.OK and got.value == 0
        text = explain(p)
        assert jt + "Join" in text and "fused" not in text and "q3" not in text, text


def test_semi_plan_splits_into_three_stages_that_each_explain():
    from flock_amd.runtime import explain
    from flock_amd.stages import build_query_dag
    for jt in ("Semi", "Anti"):
        stages = build_query_dag(_semi_plan(jt, [("i", "i_r"), ("s", "s_r")], parts=8))
        assert len(stages) == 3 and stages[0].is_shuffling and stages[1].is_shuffling and sorted(stages[2].inputs) == [0, 1]
        texts = [explain(st.plan) for st in stages]
        assert texts[2].splitlines()[0].startswith(jt + "Join [") and "_r:" not in texts[2].splitlines()[0]
        inner = build_query_dag(_semi_plan("Inner", [("i", "i_r"), ("s", "s_r")], parts=8))
        assert [s.inputs for s in stages] == [s.inputs for s in inner] and [s.node for s in stages] == [s.node for s in inner]


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def _run(gpu, plan, left, right, chunk=5_000, lcols=COLS, rcols=RCOLS):
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        return collect(ctx, [[_batches(left, chunk, lcols)], [_batches(right, chunk, rcols)]])[0][0]
    finally:
        ctx.close()


def _check_both(gpu, on, left, right, chunk=5_000, mode="Partitioned", expect_some=True):
    """Semi and Anti of one pair of tables, row for row in left order; returns the two row lists."""
    got = {}
    for jt in ("Semi", "Anti"):
        out = _run(gpu, _semi_plan(jt, on, mode=mode), left, right, chunk)
        want = _want(left, right, on, jt == "Anti")
        assert out.schema.names == NAMES, (jt, out.schema.names)
        rows = _pyrows(out)
        assert len(rows) == len(want), (jt, on, len(rows), len(want))
        assert rows == want, (jt, on)
        got[jt] = rows
    if expect_some:
        assert got["Semi"] and got["Anti"], (on, len(got["Semi"]), len(got["Anti"]))
    return got


SHAPES = {
    "i32_dense": [("i", "i_r")],
    "i64_sparse": [("l", "l_r")],                 # keys 1e9 apart: far beyond 16x the rows
    "u64_high": [("u", "u_r")],                   # keys on both sides of 2^63 (the products wrap mod 2^64)
    "timestamp": [("t", "t_r")],
    "utf8": [("s", "s_r")],                       # "" and 70-byte values among them
    "i32_pair": [("i", "i_r"), ("i2", "i2_r")],
    "i32_ts": [("i", "i_r"), ("t", "t_r")],
    "utf8_i32_i64": [("s", "s_r"), ("i", "i_r"), ("l", "l_r")],
    "eight": [(c, c + "_r") for c in NAMES[:8]],
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("nl,nr", [(300, 120), (20_000, 9_000)])
def test_key_shapes_without_nulls(gpu, shape, nl, nr):
    left, right = _pair(nl, nr, 11 * nl + nr)
    assert "" in left["s"] and any(len(x) >= 70 for x in left["s"])
    _check_both(gpu, SHAPES[shape], left, right)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("null_l,null_r", [(0.15, 0.0), (0.0, 0.15), (0.15, 0.15)])
def test_null_keys_on_either_side(gpu, shape, null_l, null_r):
    """A NULL in any key column equals nothing: NULL-keyed right rows never match, NULL-keyed left rows are dropped by Semi and KEPT by Anti."""
    on = SHAPES[shape]
    left, right = _pair(12_000, 7_000, 5, null_l=null_l, null_r=null_r)
    got = _check_both(gpu, on, left, right, chunk=4_000)
    if null_l:
        key_at = [NAMES.index(a) for a, _ in on]
        assert any(any(r[k] is None for k in key_at) for r in got["Anti"])          # they are in the Anti result ...
        assert not any(any(r[k] is None for k in key_at) for r in got["Semi"])      # ... and in no Semi result
    assert any(r[NAMES.index("f")] is None for r in got["Anti"]) and any(r[NAMES.index("f")] is None for r in got["Semi"])   # NULLs of a payload column pass through


@pytest.mark.gpu
@pytest.mark.parametrize("on", [[("i", "i_r")], [("s", "s_r")], [("i", "i_r"), ("l", "l_r")]], ids=["i32", "utf8", "two"])
def test_all_null_key_column(gpu, on):
    left, right = _pair(9_000, 3_000, 8)
    none_l, none_r = dict(left), dict(right)
    none_l[on[0][0]] = [None] * 9_000
    none_r[on[0][1]] = [None] * 3_000
    a = _check_both(gpu, on, none_l, right, expect_some=False)
    assert a["Semi"] == [] and len(a["Anti"]) == 9_000
    b = _check_both(gpu, on, left, none_r, expect_some=False)
    assert b["Semi"] == [] and len(b["Anti"]) == 9_000


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["i32_dense", "i64_sparse", "utf8", "utf8_i32_i64"])
def test_duplicates_hot_key_and_repeated_left_keys(gpu, shape):
    """One key takes half of the right rows; the left side repeats every key many times: each left row is judged on its own and appears once."""
    left = _table(15_000, 3, 40)
    right = _table(10_000, 4, 20, hot=0.5)
    right = {c + "_r": v for c, v in right.items()}
    assert right["i_r"].count(right["i_r"][[k for k in range(10_000) if right["l2_r"][k] == 7 % 5 - 2][0]]) > 10
    got = _check_both(gpu, SHAPES[shape], left, right)
    assert len(got["Semi"]) + len(got["Anti"]) == 15_000


@pytest.mark.gpu
@pytest.mark.parametrize("ty", ["Int32", "Int64"])
def test_sparse_keys_over_several_tiles_with_left_nulls(gpu, ty):
    """Ids scrambled as id * 2654435761 mod 2^32: no dense range covers them, so the hashed key set answers -- here over full tiles of the left side
    (5 tiles + 77 rows), for Int32 keys and for the same values as Int64, with NULL keys on the left."""
    from flock_amd.runtime import ExecutionContext, collect
    r = np.random.default_rng(17)
    nl, nr = 5 * TILE + 77, 12_000
    scr = lambda x: (x.astype(np.uint32) * np.uint32(2654435761)).view(np.int32).astype(np.int64)
    lk, rk = scr(r.integers(0, 40_000, nl)), scr(r.integers(0, 20_000, nr))
    assert int(rk.max()) - int(rk.min()) > 16 * nr
    null = r.random(nl) < 0.1
    pt = pa.int32() if ty == "Int32" else pa.int64()
    lcols, rcols = [("k", ty), ("row", "Int64")], [("k_r", ty)]
    lb = pa.record_batch([pa.array(lk, pt, mask=null), pa.array(np.arange(nl, dtype=np.int64))], names=["k", "row"])
    rb = pa.record_batch([pa.array(rk, pt)], names=["k_r"])
    left = {"k": [None if m else int(x) for x, m in zip(lk, null)], "row": list(range(nl))}
    right = {"k_r": [int(x) for x in rk]}
    for jt in ("Semi", "Anti"):
        ctx = ExecutionContext([_semi_plan(jt, [("k", "k_r")], lcols, rcols)], gpu=gpu)
        try:
            out = collect(ctx, [[[lb.slice(0, 2 * TILE + 3), lb.slice(2 * TILE + 3)]], [[rb]]])[0][0]
        finally:
            ctx.close()
        keep = semi_anti_rows(left, right, [("k", "k_r")], jt == "Anti")
        assert 0 < len(keep) < nl and out.column(1).to_pylist() == keep and out.column(0).to_pylist() == [left["k"][k] for k in keep], (ty, jt)
        if jt == "Anti":
            assert out.column(0).null_count == int(null.sum()) > 0


def _np_pair(nl, nr, seed):
    """Int32 key + Int64 payload tables straight from numpy (the large cases): the left keys spread over twice the right side's range."""
    r = np.random.default_rng(seed)
    k = max(1, min(nl, nr) // 3) if min(nl, nr) > 0 else 5
    lk, rk = r.integers(0, 2 * k, nl).astype(np.int32), r.integers(0, k, nr).astype(np.int32)
    lv = np.arange(nl, dtype=np.int64)
    lb = pa.record_batch([pa.array(lk), pa.array(lv)], names=["i", "v"])
    rb = pa.record_batch([pa.array(rk), pa.array(np.zeros(nr, dtype=np.int64))], names=["i_r", "v_r"])
    return {"i": lk.tolist(), "v": lv.tolist()}, {"i_r": rk.tolist(), "v_r": [0] * nr}, lb, rb


NPL, NPR = [("i", "Int32"), ("v", "Int64")], [("i_r", "Int32"), ("v_r", "Int64")]


@pytest.mark.gpu
@pytest.mark.parametrize("nl,nr", [(12, 5), (5, 40), (3 * TILE + 5, 1_000), (200 * TILE + 1, 10), (200 * TILE + 1, 4 * (200 * TILE + 1)), (0, 500), (700, 0)],
                         ids=["tiny", "tiny_right_larger", "3tiles+5", "200tiles+1_vs_10", "200tiles+1_vs_4x", "empty_left", "empty_right"])
def test_sizes(gpu, nl, nr):
    from flock_amd.runtime import ExecutionContext, collect
    left, right, lb, rb = _np_pair(nl, nr, nl + 3 * nr)
    for jt in ("Semi", "Anti"):
        ctx = ExecutionContext([_semi_plan(jt, [("i", "i_r")], NPL, NPR)], gpu=gpu)
        try:
            chunks = lambda b: [b.slice(a, max(1, b.num_rows // 3 + 1)) for a in range(0, max(b.num_rows, 1), max(1, b.num_rows // 3 + 1))]
            out = collect(ctx, [[chunks(lb)], [chunks(rb)]])[0][0]
        finally:
            ctx.close()
        keep = semi_anti_rows(left, right, [("i", "i_r")], jt == "Anti")
        assert out.num_rows == len(keep), (jt, nl, nr)
        assert out.column(1).to_pylist() == keep and out.column(0).to_pylist() == [left["i"][k] for k in keep], (jt, nl, nr)
        if nr == 0:
            assert len(keep) == (nl if jt == "Anti" else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("jt", ["Semi", "Anti"])
@pytest.mark.parametrize("shape", ["i32_dense", "i64_sparse", "utf8_i32_i64"])
def test_execute_twice_and_again_after_reset(gpu, jt, shape):
    """Cached statistics and row lists of one plan must not leak into the next execute: the same feed twice, then a reset and another feed."""
    from flock_amd.runtime import ExecutionContext
    on = SHAPES[shape]
    ctx = ExecutionContext([_semi_plan(jt, on)], gpu=gpu)
    try:
        left, right = _pair(30_000, 12_000, 21, null_l=0.1)
        ctx.feed_data_sources([[_batches(left, 7_000)], [_batches(right, 5_000, RCOLS)]])
        first, second = ctx.execute()[0][0], ctx.execute()[0][0]
        want = _want(left, right, on, jt == "Anti")
        assert _pyrows(first) == want and first.equals(second)
        ctx.clean_data_sources()
        left2, right2 = _pair(9_000, 40_000, 22, null_r=0.1)
        left2["i"] = [None if x is None else x + 70_000 * (k % 2) for k, x in enumerate(left2["i"])]      # another key range than the first feed's
        ctx.feed_data_sources([[_batches(left2, 9_000)], [_batches(right2, 11_000, RCOLS)]])
        assert _pyrows(ctx.execute()[0][0]) == _want(left2, right2, on, jt == "Anti")
        ctx.clean_data_sources()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("jt", ["Semi", "Anti"])
@pytest.mark.parametrize("where", ["left", "right", "both"])
def test_filter_under_the_inputs(gpu, jt, where):
    on = [("i", "i_r")]
    left, right = _pair(25_000, 11_000, 31, null_l=0.1)
    plan = _semi_plan(jt, on, lpred=_ge0("v", COLS) if where != "right" else None, rpred=_ge0("v_r", RCOLS) if where != "left" else None)
    fl = {c: [x for x, v in zip(col, left["v"]) if v >= 0] for c, col in left.items()} if where != "right" else left
    fr = {c: [x for x, v in zip(col, right["v_r"]) if v >= 0] for c, col in right.items()} if where != "left" else right
    want = _want(fl, fr, on, jt == "Anti")
    assert 0 < len(want) < 25_000 and _pyrows(_run(gpu, plan, left, right)) == want


THIRD = [(c + "_c", t) for c, t in COLS]


def _inner_rows(a, acols, b, bcols, ka, kb):
    """Inner join of two row-tuple lists on one column each (NULL never matches), as a multiset."""
    ia, ib = [n for n, _ in acols].index(ka), [n for n, _ in bcols].index(kb)
    by = {}
    for r in b:
        if r[ib] is not None:
            by.setdefault(r[ib], []).append(r)
    return [x + y for x in a if x[ia] is not None for y in by.get(x[ia], [])]


@pytest.mark.gpu
@pytest.mark.parametrize("jt", ["Semi", "Anti"])
@pytest.mark.parametrize("side", ["left", "right"])
def test_semi_under_an_inner_join(gpu, jt, side):
    """The Semi / Anti node goes up as a row list (exec_lazy); the Inner join above reads its key through it and takes the payload once."""
    from flock_amd.runtime import ExecutionContext, collect
    left, right = _pair(6_000, 2_500, 41, null_l=0.1)
    third = {c + "_c": v for c, v in _table(900, 43, 700).items()}
    semi = _semi_plan(jt, [("i", "i_r")])
    tscan = _coalesce(_hash(_scan(THIRD), "l2_c", THIRD))
    if side == "left":
        plan = _join("Inner", semi, tscan, COLS, THIRD, [("l2", "l2_c")], mode="CollectLeft")
    else:
        plan = _join("Inner", tscan, semi, THIRD, COLS, [("l2_c", "l2")], mode="CollectLeft")
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        srcs = [[_batches(left, 2_000)], [_batches(right, 2_000, RCOLS)], [_batches(third, 900, THIRD)]]
        out = collect(ctx, srcs)[0][0]
    finally:
        ctx.close()
    kept = _want(left, right, [("i", "i_r")], jt == "Anti")
    trows = table_rows(third, [c for c, _ in THIRD])
    want = _inner_rows(kept, COLS, trows, THIRD, "l2", "l2_c") if side == "left" else _inner_rows(trows, THIRD, kept, COLS, "l2_c", "l2")
    assert len(want) > 0 and _multiset(_pyrows(out)) == _multiset(want)


@pytest.mark.gpu
def test_anti_over_a_semi(gpu):
    left, right = _pair(14_000, 6_000, 51, null_l=0.1)
    third = {c + "_c": v for c, v in _table(5_000, 53, 2_000, null_p=0.1).items()}
    semi = _semi_plan("Semi", [("i", "i_r")])
    plan = _join("Anti", semi, _coalesce(_hash(_scan(THIRD), "s_c", THIRD)), COLS, THIRD, [("s", "s_c"), ("l", "l_c")])
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        out = collect(ctx, [[_batches(left, 5_000)], [_batches(right, 5_000, RCOLS)], [_batches(third, 5_000, THIRD)]])[0][0]
    finally:
        ctx.close()
    inner = semi_anti_table(left, right, [("i", "i_r")], False)
    want = _want(inner, third, [("s", "s_c"), ("l", "l_c")], True)
    assert 0 < len(want) < len(inner["i"]) and _pyrows(out) == want


@pytest.mark.gpu
@pytest.mark.parametrize("jt", ["Semi", "Anti"])
def test_semi_under_sort_and_limit(gpu, jt):
    left, right = _pair(18_000, 7_000, 61, null_l=0.1)
    sort = {"execution_plan": "sort_exec", "input": _semi_plan(jt, [("t", "t_r")]),
            "expr": [{"expr": _c("v"), "options": {"descending": True, "nulls_first": False}}]}
    plan = {"execution_plan": "global_limit_exec", "input": sort, "limit": 500}
    kept = _want(left, right, [("t", "t_r")], jt == "Anti")
    want = sorted(kept, key=lambda r: -r[NAMES.index("v")])[:500]            # (stable: ties in input order)
    assert _pyrows(_run(gpu, plan, left, right)) == want


@pytest.mark.gpu
@pytest.mark.parametrize("jt", ["Semi", "Anti"])
def test_semi_as_the_input_of_a_group_by(gpu, jt):
    left, right = _pair(16_000, 6_000, 71)
    cnt = {"aggregate_expr": "count", "name": "COUNT(UInt8(1))", "data_type": "UInt64", "nullable": True, "expr": {"physical_expr": "literal", "value": {"UInt8": 1}}}
    sm = {"aggregate_expr": "sum", "name": "SUM(v)", "data_type": "Int64", "nullable": True, "expr": _c("v")}
    inschema = {"fields": _fields(), "metadata": {}}
    pfields = [_field("i2", "Int32"), _field("COUNT(UInt8(1))[count]", "UInt64"), _field("SUM(v)[sum]", "Int64")]
    part = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [[_c("i2"), "i2"]], "aggr_expr": [cnt, sm],
            "input": _semi_plan(jt, [("l", "l_r")]), "input_schema": inschema, "schema": {"fields": pfields, "metadata": {}}}
    rep = {"execution_plan": "repartition_exec", "input": part, "partitioning": {"Hash": [[{"physical_expr": "column", "name": "i2", "index": 0}], 4]}}
    plan = {"execution_plan": "hash_aggregate_exec", "mode": "FinalPartitioned", "group_expr": [[{"physical_expr": "column", "name": "i2", "index": 0}, "i2"]],
            "aggr_expr": [cnt, sm], "input": _coalesce(rep), "input_schema": inschema, "schema": {"fields": [], "metadata": {}}}
    kept = semi_anti_table(left, right, [("l", "l_r")], jt == "Anti")
    groups = {}
    for k, v in zip(kept["i2"], kept["v"]):
        c, s = groups.get(k, (0, 0))
        groups[k] = (c + 1, s + v)
    want = [(k, c, s) for k, (c, s) in groups.items()]
    assert len(want) > 10 and _multiset(_pyrows(_run(gpu, plan, left, right))) == _multiset(want)


@pytest.mark.gpu
@pytest.mark.parametrize("jt", ["Semi", "Anti"])
def test_filter_and_repartition_above_through_execute_partitioned(gpu, jt):
    from flock_amd.runtime import ExecutionContext
    left, right = _pair(21_000, 8_000, 81, null_l=0.1)
    plan = _coalesce(_hash(_coalesce(_filter(_semi_plan(jt, [("i", "i_r")]), _ge0("v", COLS))), "i2", COLS, parts=5))
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        ctx.feed_data_sources([[_batches(left, 6_000)], [_batches(right, 6_000, RCOLS)]])
        parts = ctx.execute_partitioned()[0]
        ctx.clean_data_sources()
    finally:
        ctx.close()
    assert len(parts) == 5
    rows = [r for p in parts for b in p for r in _pyrows(b)]
    want = [r for r in _want(left, right, [("i", "i_r")], jt == "Anti") if r[NAMES.index("v")] >= 0]
    assert len(want) > 0 and _multiset(rows) == _multiset(want)
    per_part = [{r[NAMES.index("i2")] for b in p for r in _pyrows(b)} for p in parts]
    for a in range(5):
        for b in range(a + 1, 5):
            assert not (per_part[a] & per_part[b])          # a key lives in one partition


def _auctions(n, seed):
    """The NEXMark auction relation, item_name / description included, and a bid relation that names some of its ids."""
    r = np.random.default_rng(seed)
    aid = (np.arange(n, dtype=np.int32) + 1000)
    auction = {"a_id": aid.tolist(), "item_name": ["item-%d" % x for x in r.integers(0, 10**6, n)],
               "description": [("lot %d " % x) * int(1 + x % 5) for x in r.integers(0, 10**4, n)],
               "initial_bid": r.integers(1, 10**4, n).astype(np.int32).tolist(), "reserve": r.integers(1, 10**5, n).astype(np.int32).tolist(),
               "a_date_time": (1_436_918_400_000 + np.arange(n, dtype=np.int64) * 10).tolist(), "expires": (1_436_918_500_000 + np.arange(n, dtype=np.int64) * 10).tolist(),
               "seller": r.integers(0, 1000, n).astype(np.int32).tolist(), "category": r.integers(10, 15, n).astype(np.int32).tolist()}
    nb = 3 * n
    bid = {"auction": (r.integers(0, n // 2 + n // 8, nb) * 2 + 1000).astype(np.int32).tolist(), "bidder": r.integers(0, 500, nb).astype(np.int32).tolist(),
           "price": r.integers(1, 10**6, nb).astype(np.int32).tolist(), "b_date_time": (1_436_918_400_000 + np.arange(nb, dtype=np.int64)).tolist()}
    return auction, bid


ACOLS = [("a_id", "Int32"), ("item_name", "Utf8"), ("description", "Utf8"), ("initial_bid", "Int32"), ("reserve", "Int32"), ("a_date_time", "ts"), ("expires", "ts"),
         ("seller", "Int32"), ("category", "Int32")]
BCOLS = [("auction", "Int32"), ("bidder", "Int32"), ("price", "Int32"), ("b_date_time", "ts")]


@pytest.mark.gpu
@pytest.mark.parametrize("jt", ["Semi", "Anti"])
def test_auctions_with_and_without_bids_carry_their_text(gpu, jt):
    """auction [anti] semi join bid ON a_id = auction: the Utf8 payload (item_name, description) of the kept auctions, in auction order."""
    auction, bid = _auctions(20_000, 91)
    plan = _semi_plan(jt, [("a_id", "auction")], ACOLS, BCOLS)
    out = _run(gpu, plan, auction, bid, chunk=8_000, lcols=ACOLS, rcols=BCOLS)
    want = table_rows(semi_anti_table(auction, bid, [("a_id", "auction")], jt == "Anti"), [c for c, _ in ACOLS])
    assert 0 < len(want) < 20_000 and _pyrows(out) == want


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["i32_dense", "i64_sparse"])
def test_semi_and_anti_partition_a_million_left_rows(gpu, shape):
    """Property: the Semi rows and the Anti rows are disjoint and, merged by row position, they are the left input."""
    from flock_amd.runtime import ExecutionContext, collect
    n = 1_000_000
    r = np.random.default_rng(7)
    mul = 1 if shape == "i32_dense" else 1_000_003
    ty = pa.int32() if shape == "i32_dense" else pa.int64()
    key = r.integers(0, 400_000, n) * mul
    null = r.random(n) < 0.05
    rkey = r.integers(0, 200_000, 300_000) * mul
    lcols, rcols = [("k", "Int32" if mul == 1 else "Int64"), ("row", "Int64")], [("k_r", "Int32" if mul == 1 else "Int64")]
    lb = pa.record_batch([pa.array(key, ty, mask=null), pa.array(np.arange(n, dtype=np.int64))], names=["k", "row"])
    rb = pa.record_batch([pa.array(rkey, ty)], names=["k_r"])
    pos = {}
    for jt in ("Semi", "Anti"):
        ctx = ExecutionContext([_semi_plan(jt, [("k", "k_r")], lcols, rcols)], gpu=gpu)
        try:
            out = collect(ctx, [[[lb]], [[rb]]])[0][0]
        finally:
            ctx.close()
        pos[jt] = out.column(1).to_numpy()
        assert np.all(np.diff(pos[jt]) > 0)                                              # left order, every row at most once
        assert out.column(0).equals(lb.column(0).take(pa.array(pos[jt])))               # the rows themselves, NULL keys included
    assert len(np.intersect1d(pos["Semi"], pos["Anti"])) == 0
    assert np.array_equal(np.sort(np.concatenate([pos["Semi"], pos["Anti"]])), np.arange(n))
    present = np.isin(key, rkey) & ~null
    assert np.array_equal(pos["Semi"], np.nonzero(present)[0]) and int(null.sum()) > 0 and np.all(np.isin(np.nonzero(null)[0], pos["Anti"]))


@pytest.mark.gpu
@pytest.mark.parametrize("jt", ["Semi", "Anti"])
@pytest.mark.parametrize("how", ["eight_partitions", "one_instance_shared", "on_device"])
def test_staged_runs_equal_the_whole_plan(gpu, jt, how):
    """The plan split at its join (build_query_dag): two shuffling stages, then the join over their partitions -- the union of the stages' results
    equals the whole plan's equals the reference's, NULL-keyed left rows present under Anti."""
    from flock_amd import stages as S
    on = [("i", "i_r"), ("s", "s_r")]
    left, right = _pair(24_000, 9_000, 101, null_l=0.1, null_r=0.1)
    plan = _semi_plan(jt, on, parts=8)
    lb, rb = _batches(left, 24_000)[0], _batches(right, 9_000, RCOLS)[0]
    whole = _pyrows(_run(gpu, plan, left, right, chunk=7_000))
    want = _want(left, right, on, jt == "Anti")
    assert whole == want
    stages = S.build_query_dag(plan)
    assert len(stages) == 3
    kw = {"eight_partitions": dict(chunks=2), "one_instance_shared": dict(instances=1, share_sources=True), "on_device": dict(on_device=True)}[how]
    run = S.StagedRun(gpu, stages, **kw)
    try:
        out = run.run({"left": lb, "right": rb})
    finally:
        run.close()
    out = out if isinstance(out, list) else [out]
    rows = [r for b in out for r in _pyrows(b)]
    assert _multiset(rows) == _multiset(want)
    if jt == "Anti":
        assert any(r[0] is None or r[NAMES.index("s")] is None for r in rows)


@pytest.mark.gpu
@pytest.mark.parametrize("jt", ["Semi", "Anti"])
def test_q3_look_alike_runs_on_the_generic_operators(gpu, jt):
    from flock_amd.runtime import ExecutionContext, collect
    r = np.random.default_rng(3)
    n_person, n_auction = 30_000, 90_000
    states = ["or", "id", "ca", "oh", "ok", "wa"]
    person = {"p_id": (np.arange(n_person, dtype=np.int32) + 1000).tolist(), "name": ["n%d" % k for k in range(n_person)], "city": ["c%d" % (k % 97) for k in range(n_person)],
              "state": [states[int(j)] for j in r.integers(0, len(states), n_person)]}
    auction = {"a_id": (np.arange(n_auction, dtype=np.int32) + 5000).tolist(), "seller": (r.integers(0, n_person + 5_000, n_auction) + 1000).astype(np.int32).tolist(),
               "category": r.integers(8, 13, n_auction).astype(np.int32).tolist()}
    pb = pa.record_batch([pa.array(person["p_id"], pa.int32()), pa.array(person["name"]), pa.array(person["city"]), pa.array(person["state"])], names=list(person))
    ab = pa.record_batch([pa.array(auction[c], pa.int32()) for c in auction], names=list(auction))
    ctx = ExecutionContext([_q3_semi(jt)], gpu=gpu)
    try:
        out = collect(ctx, [[[ab]], [[pb]]])[0][0]
    finally:
        ctx.close()
    fa = {c: [x for x, cat in zip(v, auction["category"]) if cat == 10] for c, v in auction.items()}
    fp = {c: [x for x, st in zip(v, person["state"]) if st in ("or", "id", "ca")] for c, v in person.items()}
    want = table_rows(semi_anti_table(fa, fp, [("seller", "p_id")], jt == "Anti"), ["a_id", "seller"])
    assert len(want) > 1_000 and out.schema.names == ["a_id", "seller"] and _pyrows(out) == want
