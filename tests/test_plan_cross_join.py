"""CrossJoinExec (cross.hpp A-X1..6): the left input's columns followed by the right input's, L x R rows, pair (i, j) at output row i * R + j -- against
the plain-Python reference of tests/cross_join_ref.py, row for row IN ORDER, validity included (floats by their bits)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pyarrow as pa
import pytest

from cross_join_ref import cross_rows, cross_table, rows_of
from oracle import generic_ops as ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")


def _header_int(name):
    text = open(os.path.join(ROOT, "flock_amd", "csrc", "cross.hpp")).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))


CHUNKS = _header_int("kCrossTileChunks")     # 16-byte output chunks of one workgroup
ROWS4, ROWS8 = CHUNKS * 4, CHUNKS * 2        # rows of one workgroup of the 4-byte / 8-byte kernels (validity bytes: CHUNKS * 16)

_TS = {"Timestamp": ["Millisecond", None]}
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string(), "ts": pa.timestamp("ms")}
# every type the boundary carries, two Utf8 columns, and `z`: a column that is nothing but NULLs
COLS = [("i", "Int32"), ("l", "Int64"), ("u", "UInt64"), ("t", "ts"), ("f", "Float64"), ("s", "Utf8"), ("s2", "Utf8"), ("z", "Int32")]
RCOLS = [(c + "_r", t) for c, t in COLS]
NAMES, RNAMES = [c for c, _ in COLS], [c for c, _ in RCOLS]
WORDS = ["", "a", "ab", "abc", "x" * 17, "y" * 17 + "z", "w" * 70, "w" * 69 + "v", "été", "key"]     # (the semi-join tests' word list)
FLOATS = [float("inf"), float("-inf"), -0.0, 0.0, 1.5, -2.25e300, 4.9e-324]


# ------------------------------------------------------------------ plans
def _dt(t):
    return _TS if t == "ts" else t


def _field(name, t, nullable=True):
    return {"data_type": _dt(t), "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


def _fields(cols):
    return [_field(n, t) for n, t in cols]


def _schema(cols):
    return {"fields": _fields(cols), "metadata": {}}


def _c(name, cols):
    return {"physical_expr": "column", "name": name, "index": [n for n, _ in cols].index(name)}


def _lit(ty, v):
    return {"physical_expr": "literal", "value": {ty: v}}


def _bin(l, op, r):
    return {"physical_expr": "binary_expr", "left": l, "op": op, "right": r}


def _cast(e, ty):
    return {"physical_expr": "cast_expr", "expr": e, "cast_type": ty}


def _scan(cols):
    return {"execution_plan": "memory_exec", "schema": _schema(cols), "projection": list(range(len(cols)))}


def _filter(inp, pred):
    return {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096, "input": {"execution_plan": "filter_exec", "predicate": pred, "input": inp}}


def _project(inp, exprs, cols):
    return {"execution_plan": "projection_exec", "expr": [[e, n] for e, n in exprs], "input": inp, "schema": _schema(cols)}


def _cross(left, right, lcols, rcols, **extra):
    p = {"execution_plan": "cross_join_exec", "left": left, "right": right, "schema": _schema(list(lcols) + list(rcols))}
    p.update(extra)
    return p


def _count_star():
    return {"aggregate_expr": "count", "name": "COUNT(UInt8(1))", "data_type": "UInt64", "nullable": True, "expr": _lit("UInt8", 1)}


def _agg(mode, group, entries, inp, in_cols, out_cols):
    return {"execution_plan": "hash_aggregate_exec", "mode": mode, "group_expr": group, "aggr_expr": entries, "input": inp, "input_schema": _schema(in_cols),
            "schema": _schema(out_cols)}


def _state_cols(entries):
    out = []
    for e in entries:
        if e["aggregate_expr"] == "avg":
            out += [(e["name"] + "[count]", "UInt64"), (e["name"] + "[sum]", "Float64")]
        else:
            out.append(("%s[%s]" % (e["name"], e["aggregate_expr"]), e["data_type"]))
    return out


def _ungrouped(entries, inp, in_cols):
    """Partial -> CoalescePartitions -> Final, as the planner writes SELECT <aggregates> FROM ..."""
    part = _agg("Partial", [], entries, inp, in_cols, _state_cols(entries))
    return _agg("Final", [], entries, {"execution_plan": "coalesce_partitions_exec", "input": part}, in_cols, [(e["name"], e["data_type"]) for e in entries])


def _entry(fn, name, ty, expr):
    return {"aggregate_expr": fn, "name": name, "data_type": _dt(ty), "nullable": True, "expr": expr}


# ------------------------------------------------------------------ tables: {name: list of Python values, None = NULL}
def make_table(n, seed, null_p=0.0, suffix=""):
    r = np.random.default_rng(seed)
    t = {"i": [int(x) for x in r.integers(-2**31, 2**31, n)],
         "l": [int(x) for x in r.integers(-2**62, 2**62, n)],
         "u": [2**63 + int(x) for x in r.integers(0, 2**62, n)],                                   # every value at or above 2^63
         "t": [1_436_918_400_000 + int(x) for x in r.integers(0, 10**9, n)],
         "f": [FLOATS[k % len(FLOATS)] if k % 3 else float(np.round(r.normal(0, 1e6), 3)) for k in range(n)],
         "s": [WORDS[int(x)] for x in r.integers(0, len(WORDS), n)],
         "s2": [WORDS[(k * 3 + 1) % len(WORDS)] + ("%d" % k if k % 4 == 0 else "") for k in range(n)],
         "z": [None] * n}
    if null_p > 0:
        for c in ("i", "l", "u", "t", "f", "s", "s2"):
            m = r.random(n) < null_p
            t[c] = [None if m[k] else t[c][k] for k in range(n)]
    return {c + suffix: v for c, v in t.items()}


def _batches(t, chunk, cols):
    n = len(t[cols[0][0]])
    return [pa.record_batch([pa.array(t[c][a:a + chunk], _PA[ty]) for c, ty in cols], names=[c for c, _ in cols]) for a in range(0, max(n, 1), max(chunk, 1))]


def _bits(v):
    return ("f", np.float64(v).view(np.uint64).item()) if isinstance(v, float) else v


def _norm(rows):
    """floats by their bits: -0.0 is not 0.0, and an infinity is itself"""
    return [tuple(_bits(v) for v in r) for r in rows]


def _pyrows(rb):
    cols = []
    for i in range(rb.num_columns):
        c = rb.column(i)
        if pa.types.is_timestamp(c.type):
            c = c.cast(pa.int64())
        cols.append(c.to_pylist())
    return _norm(zip(*cols)) if cols else []


def _buffers(rb):
    """every buffer of every column as bytes (validity bitmap, offsets, values): what "byte-identical output" compares"""
    out = []
    for i in range(rb.num_columns):
        c = rb.column(i)
        out.append((str(c.type), len(c), c.null_count, tuple(None if b is None else b.to_pybytes() for b in c.buffers())))
    return out


@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def _run(gpu, plan, feeds, executes=1):
    """feeds: per leaf a list of batches; the one output batch (of the last execute)"""
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        for _ in range(executes):
            out = collect(ctx, [[f] for f in feeds])[0]
    finally:
        ctx.close()
    assert len(out) == 1
    return out[0]


def _check_cross(gpu, left, right, chunk=5_000, lcols=COLS, rcols=RCOLS):
    out = _run(gpu, _cross(_scan(lcols), _scan(rcols), lcols, rcols), [_batches(left, chunk, lcols), _batches(right, chunk, rcols)])
    ln, rn = [c for c, _ in lcols], [c for c, _ in rcols]
    assert out.schema.names == ln + rn
    want = _norm(cross_rows(rows_of(left, ln), rows_of(right, rn)))
    got = _pyrows(out)
    assert len(got) == len(want) == len(left[ln[0]]) * len(right[rn[0]])
    assert got == want
    return out


# ------------------------------------------------------------------ CPU: the reference itself
def test_reference_on_hand_worked_rows():
    left, right = [(1, "a"), (None, "b")], [(10.5,), (None,), (-0.0,)]
    assert cross_rows(left, right) == [(1, "a", 10.5), (1, "a", None), (1, "a", -0.0), (None, "b", 10.5), (None, "b", None), (None, "b", -0.0)]
    assert cross_rows([], right) == [] and cross_rows(left, []) == []
    assert cross_rows(cross_rows([(1,), (2,)], [(3,)]), [(4,), (5,)]) == cross_rows([(1,), (2,)], cross_rows([(3,)], [(4,), (5,)]))     # A-X2 composes
    assert cross_table({"a": [1, 2]}, {"b": ["x", "y", "z"]}) == {"a": [1, 1, 1, 2, 2, 2], "b": ["x", "y", "z", "x", "y", "z"]}
    assert cross_table({"a": []}, {"b": ["x"]}) == {"a": [], "b": []}


def test_host_index_helpers_under_the_sanitizers():
    """cross.hpp's host-callable helpers (quotient / remainder by the reciprocal, the A-X6 checks, the closed-form offsets) in a stand-alone program built
    with AddressSanitizer and UBSan -- host code on the CPU, nothing of it is loaded into Python."""
    import subprocess
    exe = os.path.join(ROOT, "tests", "cpp", "cross_index_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "flock_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "cross_index_test.cpp"), "-o", exe])
    assert "cross_index_test ok" in subprocess.check_output([exe], text=True)


# ------------------------------------------------------------------ CPU: parsing, recognition, pruning, stage split
def test_explain_prints_crossjoin_over_scans_with_left_then_right_columns():
    from flock_amd.runtime import explain
    lines = explain(_cross(_scan(COLS), _scan(RCOLS), COLS, RCOLS)).splitlines()
    assert lines[0].startswith("CrossJoin [") and lines[1].strip().startswith("Scan") and lines[2].strip().startswith("Scan") and len(lines) == 3, lines
    head = lines[0][lines[0].index("[") + 1:lines[0].index("]")]
    assert [x.split(":")[0] for x in head.split(", ")] == NAMES + RNAMES
    assert [x.split(":")[1] for x in head.split(", ")] == ["Int32", "Int64", "UInt64", "Timestamp(ms)", "Float64", "Utf8", "Utf8", "Int32"] * 2
    bare = _cross(_scan(COLS), _scan(RCOLS), COLS, RCOLS)
    del bare["schema"]                                                   # the node's schema is optional
    assert explain(bare).splitlines()[0] == lines[0]


def test_the_fixture_parses_explains_and_is_no_fused_query():
    from flock_amd import _ffi, build
    from flock_amd.runtime import explain
    build.build()
    lib = _ffi.load()
    text = open(os.path.join(PLANS, "bids_above_average.json")).read()
    lines = explain(text).splitlines()
    assert lines[0] == "Project [auction:Int32, bidder:Int32, price:Int32, avgp:Float64]"
    assert lines[1].strip().startswith("Filter [") and lines[2].strip().startswith("CrossJoin [auction:Int32, bidder:Int32, price:Int32, avgp:Float64]"), lines
    assert "Aggregate(Final)" in "\n".join(lines) and "fused" not in "\n".join(lines)
    got = C.c_int(-1)
    raw = text.encode()
    assert lib.flockgpu_plan_recognise(raw, len(raw), C.byref(got)) == _ffi.OK and got.value == 0


def _q3_cross():
    p = json.load(open(os.path.join(PLANS, "q3.json")))
    j = p["input"]["input"]
    assert j["execution_plan"] == "hash_join_exec"
    j["execution_plan"] = "cross_join_exec"
    del j["on"]
    return p


def test_q3_look_alike_with_a_cross_join_is_not_fused():
    from flock_amd import _ffi, build
    from flock_amd.runtime import explain
    build.build()
    lib = _ffi.load()
    got = C.c_int(-1)
    raw = open(os.path.join(PLANS, "q3.json")).read().encode()
    assert lib.flockgpu_plan_recognise(raw, len(raw), C.byref(got)) == _ffi.OK and got.value == 3
    p = _q3_cross()
    raw = json.dumps(p).encode()
    assert lib.flockgpu_plan_recognise(raw, len(raw), C.byref(got)) == _ffi.OK and got.value == 0
    text = explain(p)
    assert "CrossJoin" in text and "fused" not in text and "q3" not in text, text


def _refused(plan, *words):
    from flock_amd import _ffi
    from flock_amd.runtime import FlockGpuError, explain
    with pytest.raises(FlockGpuError) as e:
        explain(plan)
    assert e.value.code in (_ffi.ERR_UNSUPPORTED, _ffi.ERR_PLAN), str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals_by_name():
    short = _cross(_scan(COLS), _scan(RCOLS), COLS, RCOLS)
    short["schema"]["fields"].pop()                                       # a column missing
    _refused(short, "Cross join", "schema", "15 columns", "8 + 8")
    wrong = _cross(_scan(COLS), _scan(RCOLS), COLS, RCOLS)
    wrong["schema"]["fields"][9]["data_type"] = "Int32"                   # l_r: Int64 in the input
    _refused(wrong, "Cross join", "schema", "l_r", "Int32", "Int64")
    stamp = _cross(_scan(COLS), _scan(RCOLS), COLS, RCOLS)
    stamp["schema"]["fields"][3]["data_type"] = "Int64"                   # t: a Timestamp in the input (the same storage, another type)
    _refused(stamp, "Cross join", "schema", "'t'", "Timestamp")
    for side in ("left", "right"):
        p = _cross(_scan(COLS), _scan(RCOLS), COLS, RCOLS)
        del p[side]
        _refused(p, "malformed plan node")


def test_on_join_type_mode_and_random_state_are_ignored():
    from flock_amd.runtime import explain
    plain = explain(_cross(_scan(COLS), _scan(RCOLS), COLS, RCOLS))
    noisy = _cross(_scan(COLS), _scan(RCOLS), COLS, RCOLS, on=[], join_type="Left", mode="Partitioned", random_state={"k0": 0, "k1": 0, "k2": 0, "k3": 0})
    assert explain(noisy) == plain
    noisy["on"] = [[_c("i", COLS), _c("i_r", RCOLS)]]
    noisy["join_type"] = "Inner"
    assert explain(noisy) == plain


def _scan_reads(text):
    return [ln[ln.index("reads [") + 7:ln.rindex("]")] for ln in text.splitlines() if ln.strip().startswith("Scan")]


def test_pruning_reaches_both_leaves():
    """A-X5: COUNT(*) over a cross join asks neither leaf for a column; a projection of one column of each side asks for those two."""
    from flock_amd.runtime import explain
    x = _cross(_scan(COLS), _scan(RCOLS), COLS, RCOLS)
    assert _scan_reads(explain(x)) == [", ".join(NAMES), ", ".join(RNAMES)]
    count = _ungrouped([_count_star()], x, COLS + RCOLS)
    assert _scan_reads(explain(count)) == ["", ""]
    both = COLS + RCOLS
    two = _project(x, [(_c("s_r", both), "s_r"), (_c("l", both), "l")], [("s_r", "Utf8"), ("l", "Int64")])
    assert _scan_reads(explain(two)) == ["l", "s_r"]
    # a filter above on a left and a right column, a projection of a third: the leaves read what the filter and the projection read
    pred = _bin(_bin(_c("i", both), "Gt", _lit("Int32", 0)), "And", _bin(_c("f_r", both), "Lt", _lit("Float64", 1.0)))
    top = _project(_filter(x, pred), [(_c("t", both), "t")], [("t", "ts")])
    assert _scan_reads(explain(top)) == ["i, t", "f_r"]


def test_the_stage_splitter_does_not_cut_at_a_cross_join():
    """Final aggregate <- hash repartition <- Partial aggregate <- cross join of two scans: one cut, at the repartition; the cross join and both of
    its leaves lie in one stage (the reference's stage.rs knows no such node: its walk over input / left / right descends through it)."""
    from flock_amd.runtime import explain
    from flock_amd.stages import build_query_dag
    both = COLS + RCOLS
    x = _cross(_scan(COLS), _scan(RCOLS), COLS, RCOLS)
    cnt = _count_star()
    pf = [("i", "Int32"), ("COUNT(UInt8(1))[count]", "UInt64")]
    part = _agg("Partial", [[_c("i", both), "i"]], [cnt], x, both, pf)
    rep = {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096,
           "input": {"execution_plan": "repartition_exec", "input": part, "partitioning": {"Hash": [[{"physical_expr": "column", "name": "i", "index": 0}], 4]}}}
    fin = _agg("FinalPartitioned", [[{"physical_expr": "column", "name": "i", "index": 0}, "i"]], [cnt], rep, both, [("i", "Int32"), ("COUNT(UInt8(1))", "UInt64")])
    stages = build_query_dag(fin)
    assert len(stages) == 2, [s.node for s in stages]
    texts = [explain(st.plan) for st in stages]
    with_cross = [t for t in texts if "CrossJoin" in t]
    assert len(with_cross) == 1 and with_cross[0].count("Scan") == 2, texts
    assert [st.is_shuffling for st in stages] == [True, False] and stages[0].inputs == [None, None] and stages[1].inputs == [0]
    # a sort directly over a cross join: the cut-off input's schema is the cross join's (left ++ right), and both stages explain
    sort = {"execution_plan": "sort_exec", "input": x, "expr": [{"expr": _c("i", both), "options": {"descending": False, "nulls_first": False}}]}
    for plan in (sort, {k: v for k, v in sort.items() if k != "input"} | {"input": {k: v for k, v in x.items() if k != "schema"}}):
        st = build_query_dag(plan)
        assert len(st) == 2 and "CrossJoin" in explain(st[0].plan) and explain(st[1].plan).splitlines()[1].strip().startswith("Scan() [i:Int32, l:Int64"), st
    assert "Aggregate(FinalPartitioned)" in [t for t in texts if "CrossJoin" not in t][0]


# ------------------------------------------------------------------ GPU 1: shapes
SMALL = [(0, 0), (0, 5), (5, 0), (1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (5, 4), (4, 5), (3, 16), (16, 3), (17, 15)]
# L x R and R at a workgroup's rows +- 1 (the 4-byte kernels' and the 8-byte kernels'), and the same counts with the sides swapped; a workgroup of
# validity bytes holds CHUNKS * 16 rows: (2, ROWS8 * 4 +- 1) puts L x R next to that
AROUND = [(1, ROWS4 - 1), (1, ROWS4), (1, ROWS4 + 1), (1, ROWS8 - 1), (1, ROWS8 + 1), (ROWS4 + 1, 1), (2, ROWS8 + 1), (2, ROWS8 - 1), (ROWS8 + 1, 2), (2, ROWS8 * 4 + 1),
          (2, ROWS8 * 4 - 1)]
BIG = [(257, 263), (1, 70_001), (70_001, 1), (3, 40_003), (40_003, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("nulls", [False, True], ids=["plain", "nulls"])
@pytest.mark.parametrize("shape", SMALL + AROUND + BIG, ids=lambda s: "%dx%d" % s)
def test_every_pair_in_left_major_order(gpu, shape, nulls):
    nl, nr = shape
    left, right = make_table(nl, 7 * nl + nr, 0.3 if nulls else 0.0), make_table(nr, 11 * nr + nl + 1, 0.3 if nulls else 0.0, "_r")
    out = _check_cross(gpu, left, right, chunk=max(nl, nr, 1))
    assert out.column("s").null_count == left["s"].count(None) * nr and out.column("f_r").null_count == right["f_r"].count(None) * nl
    if nulls and min(nl, nr) >= 100:
        assert 0 < out.column("s").null_count < nl * nr and 0 < out.column("f_r").null_count < nl * nr
    assert out.column("z").null_count == nl * nr and out.column("z_r").null_count == nl * nr      # (A-X3: nothing but NULLs stays so)


# ------------------------------------------------------------------ GPU 2: batching and repeats change no byte
@pytest.mark.gpu
def test_batching_and_a_second_execute_change_no_byte(gpu):
    from flock_amd.runtime import ExecutionContext, collect
    nl, nr = 23, 19
    left, right = make_table(nl, 5, 0.3), make_table(nr, 6, 0.3, "_r")
    plan = _cross(_scan(COLS), _scan(RCOLS), COLS, RCOLS)
    seen = []
    for chunk in (max(nl, nr), 1, 7):
        ctx = ExecutionContext([plan], gpu=gpu)
        try:
            for _ in range(2):                       # (the second execute finds the first one's arenas)
                out = collect(ctx, [[_batches(left, chunk, COLS)], [_batches(right, chunk, RCOLS)]])[0]
                assert len(out) == 1
                seen.append((_buffers(out[0]), _pyrows(out[0])))
        finally:
            ctx.close()
    assert all(s[1] == seen[0][1] for s in seen)
    assert all(s[0] == seen[0][0] for s in seen)
    assert seen[0][1] == _norm(cross_rows(rows_of(left, NAMES), rows_of(right, RNAMES)))


# ------------------------------------------------------------------ GPU 3: lazy sides (a filter directly under the cross join)
def _pred(which, cols, sfx="", one=None):
    """selectivity 0, ~1/3, 1 and exactly one row (i is unique per row: the test checks); a NULL i fails every one of them"""
    i = _c("i" + sfx, cols)
    if which == "none":
        return _bin(i, "Lt", _lit("Int32", -2**31))
    if which == "third":
        return _bin(_bin(_cast(i, "Int64"), "Modulo", _lit("Int64", 3)), "Eq", _lit("Int64", 0))
    if which == "all":
        return _bin(i, "GtEq", _lit("Int32", -2**31))
    return _bin(i, "Eq", _lit("Int32", one))


def _keep(t, which, sfx="", one=None):
    col = t["i" + sfx]
    if which == "none":
        return [False] * len(col)
    if which == "all":
        return [v is not None for v in col]
    if which == "third":
        return [v is not None and v % 3 == 0 for v in col]
    return [v == one for v in col]


@pytest.mark.gpu
@pytest.mark.parametrize("lw,rw", [("third", None), (None, "third"), ("third", "third"), ("none", "all"), ("all", "none"), ("all", "all"), ("one", None), (None, "one"),
                                   ("one", "third"), ("one", "one")])
def test_a_filter_directly_under_either_side(gpu, lw, rw):
    nl, nr = 211, 157
    left, right = make_table(nl, 31), make_table(nr, 37, 0.2, "_r")
    one_l, one_r = left["i"][100], next(v for v in right["i_r"][50:] if v is not None)
    assert left["i"].count(one_l) == 1 and right["i_r"].count(one_r) == 1

    def side(scan, cols, which, sfx, one):
        if which is None:
            return scan
        return _filter(scan, _pred(which, cols, sfx, one))
    plan = _cross(side(_scan(COLS), COLS, lw, "", one_l), side(_scan(RCOLS), RCOLS, rw, "_r", one_r), COLS, RCOLS)
    out = _run(gpu, plan, [_batches(left, 64, COLS), _batches(right, 64, RCOLS)])
    kl = [True] * nl if lw is None else _keep(left, lw, "", one_l)
    kr = [True] * nr if rw is None else _keep(right, rw, "_r", one_r)
    lrows = [r for r, k in zip(rows_of(left, NAMES), kl) if k]
    rrows = [r for r, k in zip(rows_of(right, RNAMES), kr) if k]
    if lw == "third":
        assert nl // 6 < len(lrows) < nl // 2
    if lw == "one":
        assert len(lrows) == 1
    assert _pyrows(out) == _norm(cross_rows(lrows, rrows))
    assert out.num_rows == len(lrows) * len(rrows)


# ------------------------------------------------------------------ GPU 4: the aggregate row
BID = [("auction", "Int32"), ("bidder", "Int32"), ("price", "Int32"), ("b_date_time", "ts")]


def _bids(n, seed):
    r = np.random.default_rng(seed)
    return {"auction": [int(x) for x in r.integers(1000, 2000, n)], "bidder": [int(x) for x in r.integers(0, 500, n)],
            "price": [int(x) for x in r.integers(100, 10_000_000, n)], "b_date_time": [1_436_918_400_000 + 7 * k for k in range(n)]}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1000, ROWS4 * 3 + 5])
def test_the_fixture_statement_bids_above_the_average(gpu, n):
    bid = _bids(n, 41 + n)
    plan = open(os.path.join(PLANS, "bids_above_average.json")).read()
    out = _run(gpu, plan, [_batches(bid, 1500, BID)], executes=2)
    agg = ops.hash_aggregate_exec({"price": bid["price"]}, [], [("avgp", "avg", "price")])
    assert agg["avgp"] == [sum(bid["price"]) / n]                                      # (exact: an integer sum below 2^53, one division)
    three = {c: bid[c] for c in ("auction", "bidder", "price")}
    x = cross_table(three, agg)
    names = ["auction", "bidder", "price", "avgp"]
    types = {"auction": "Int32", "bidder": "Int32", "price": "Int32", "avgp": "Float64"}
    cols4 = [(c, types[c]) for c in names]
    want = ops.filter_by_typed_expr(x, _bin(_cast(_c("price", cols4), "Float64"), "Gt", _c("avgp", cols4)), types)
    assert out.schema.names == names
    assert _pyrows(out) == _norm(rows_of(want, names))
    assert (n == 1) == (out.num_rows == 0)


@pytest.mark.gpu
def test_an_aggregate_over_no_rows_gives_null_columns_and_the_filter_keeps_none(gpu):
    """(COUNT = 0, AVG = NULL) crossed with n bids: n rows whose avgp is NULL; `price > avgp` above keeps none of them."""
    n = 300
    bid = _bids(n, 43)
    acols = [("p_r", "Int32")]
    entries = [_entry("count", "COUNT(UInt8(1))", "UInt64", _lit("UInt8", 1)), _entry("avg", "AVG(p_r)", "Float64", _c("p_r", acols))]
    right = _ungrouped(entries, _scan(acols), acols)
    rcols = [("COUNT(UInt8(1))", "UInt64"), ("AVG(p_r)", "Float64")]
    x = _cross(_scan(BID), right, BID, rcols)
    empty = [pa.record_batch([pa.array([], pa.int32())], names=["p_r"])]
    out = _run(gpu, x, [_batches(bid, 100, BID), empty])
    want = cross_rows(rows_of(bid, [c for c, _ in BID]), [(0, None)])
    assert _pyrows(out) == _norm(want) and out.num_rows == n and out.column("AVG(p_r)").null_count == n
    both = BID + rcols
    kept = _filter(x, _bin(_cast(_c("price", both), "Float64"), "Gt", _c("AVG(p_r)", both)))
    assert _run(gpu, kept, [_batches(bid, 100, BID), empty]).num_rows == 0


@pytest.mark.gpu
def test_a_projection_reads_columns_of_both_sides(gpu):
    """SELECT auction, price, price - minp, maxp - minp FROM bid, (SELECT MIN(price) minp, MAX(price) maxp FROM bid2) r"""
    n = ROWS4 + 3
    bid = _bids(n, 47)
    acols = [("p_r", "Int32")]
    entries = [_entry("min", "MIN(p_r)", "Int32", _c("p_r", acols)), _entry("max", "MAX(p_r)", "Int32", _c("p_r", acols))]
    rcols = [("MIN(p_r)", "Int32"), ("MAX(p_r)", "Int32")]
    both = BID + rcols
    x = _cross(_scan(BID), _ungrouped(entries, _scan(acols), acols), BID, rcols)
    exprs = [(_c("auction", both), "auction"), (_c("price", both), "price"), (_bin(_c("price", both), "Minus", _c("MIN(p_r)", both)), "above"),
             (_bin(_c("MAX(p_r)", both), "Minus", _c("MIN(p_r)", both)), "range")]
    plan = _project(x, exprs, [("auction", "Int32"), ("price", "Int32"), ("above", "Int32"), ("range", "Int32")])
    side = {"p_r": bid["price"][::2]}
    out = _run(gpu, plan, [_batches(bid, 999, BID), _batches(side, 4096, acols)])
    lo, hi = min(side["p_r"]), max(side["p_r"])
    agg = ops.hash_aggregate_exec(side, [], [("MIN(p_r)", "min", "p_r"), ("MAX(p_r)", "max", "p_r")])
    assert rows_of(agg, ["MIN(p_r)", "MAX(p_r)"]) == [(lo, hi)]
    xt = cross_table(bid, agg)
    want = ops.project_typed(xt, exprs, dict(both))
    assert _pyrows(out) == _norm(rows_of(want, ["auction", "price", "above", "range"]))


# ------------------------------------------------------------------ GPU 5: composition
A = [("a", "Int32"), ("as", "Utf8")]
B = [("b", "Int64"), ("bs", "Utf8")]
D = [("d", "Int32"), ("df", "Float64")]


def _abd():
    a = {"a": [1, None], "as": ["x", "été"]}
    b = {"b": [10, 20, None], "bs": ["", "w" * 70, None]}
    d = {"d": [1, 2, 3, 4, 1], "df": [0.5, -0.0, None, float("inf"), 2.0]}
    return a, b, d


@pytest.mark.gpu
def test_a_three_way_cross_left_deep_and_right_deep(gpu):
    a, b, d = _abd()
    feeds = [_batches(a, 8, A), _batches(b, 8, B), _batches(d, 8, D)]
    want = _norm(cross_rows(cross_rows(rows_of(a, ["a", "as"]), rows_of(b, ["b", "bs"])), rows_of(d, ["d", "df"])))
    assert len(want) == 30
    left_deep = _cross(_cross(_scan(A), _scan(B), A, B), _scan(D), A + B, D)
    right_deep = _cross(_scan(A), _cross(_scan(B), _scan(D), B, D), A, B + D)
    assert _pyrows(_run(gpu, left_deep, feeds)) == want
    assert _pyrows(_run(gpu, right_deep, feeds)) == want


@pytest.mark.gpu
def test_under_an_inner_join_and_under_a_semi_join(gpu):
    a, b, d = _abd()
    x = _cross(_scan(A), _scan(B), A, B)
    feeds = [_batches(a, 8, A), _batches(b, 8, B), _batches(d, 8, D)]
    xt = cross_table(a, b)
    inner = {"execution_plan": "hash_join_exec", "left": x, "right": _scan(D), "join_type": "Inner", "mode": "CollectLeft", "on": [[_c("a", A + B), _c("d", D)]],
             "schema": _schema(A + B + D)}
    want = ops.hash_join_inner(xt, d, [("a", "d")])
    got = _pyrows(_run(gpu, inner, feeds))
    assert sorted(got, key=repr) == sorted(_norm(rows_of(want, [c for c, _ in A + B + D])), key=repr) and len(got) == 6
    semi = {"execution_plan": "hash_join_exec", "left": x, "right": _scan(D), "join_type": "Semi", "mode": "CollectLeft", "on": [[_c("a", A + B), _c("d", D)]],
            "schema": _schema(A + B)}
    assert _pyrows(_run(gpu, semi, feeds)) == _norm(r for r in rows_of(xt, [c for c, _ in A + B]) if r[0] == 1)


@pytest.mark.gpu
def test_under_sort_limit_group_by_and_ungrouped_aggregates(gpu):
    nl, nr = 37, 29
    left, right = make_table(nl, 61), make_table(nr, 67, 0.0, "_r")
    both = COLS + RCOLS
    x = _cross(_scan(COLS), _scan(RCOLS), COLS, RCOLS)
    feeds = [_batches(left, 16, COLS), _batches(right, 16, RCOLS)]
    xt = cross_table(left, right)
    # ORDER BY i_r DESC, i ASC LIMIT 50 (both unique per source row: no ties)
    assert len(set(left["i"])) == nl and len(set(right["i_r"])) == nr
    sort = {"execution_plan": "sort_exec", "input": x, "expr": [{"expr": _c("i_r", both), "options": {"descending": True, "nulls_first": False}},
                                                               {"expr": _c("i", both), "options": {"descending": False, "nulls_first": False}}]}
    lim = {"execution_plan": "global_limit_exec", "input": sort, "limit": 50}
    want = ops.limit_exec(ops.sort_exec(xt, [("i_r", True), ("i", False)]), 50)
    assert _pyrows(_run(gpu, lim, feeds)) == _norm(rows_of(want, NAMES + RNAMES))
    # COUNT(*) = L x R without a column; SUM of a left and of a right column
    entries = [_count_star(), _entry("sum", "SUM(i)", "Int64", _c("i", both)), _entry("sum", "SUM(t_r)", "Int64", _c("t_r", both))]
    out = _run(gpu, _ungrouped(entries, x, both), feeds)
    assert [c.to_pylist()[0] for c in out.columns] == [nl * nr, nr * sum(left["i"]), nl * sum(right["t_r"])]
    only_count = _run(gpu, _ungrouped([_count_star()], x, both), feeds)
    assert only_count.column(0).to_pylist() == [nl * nr]
    # GROUP BY s (a left Utf8 column): COUNT(*), MAX(l_r)
    cnt, mx = _count_star(), _entry("max", "MAX(l_r)", "Int64", _c("l_r", both))
    part = _agg("Partial", [[_c("s", both), "s"]], [cnt, mx], x, both, [("s", "Utf8"), ("COUNT(UInt8(1))[count]", "UInt64"), ("MAX(l_r)[max]", "Int64")])
    rep = {"execution_plan": "repartition_exec", "input": part, "partitioning": {"Hash": [[{"physical_expr": "column", "name": "s", "index": 0}], 4]}}
    fin = _agg("FinalPartitioned", [[{"physical_expr": "column", "name": "s", "index": 0}, "s"]], [cnt, mx], rep, both,
               [("s", "Utf8"), ("COUNT(UInt8(1))", "UInt64"), ("MAX(l_r)", "Int64")])
    want = ops.hash_aggregate_exec(xt, ["s"], [("n", "count", None), ("m", "max", "l_r")])
    got = _run(gpu, fin, feeds)
    assert sorted(_pyrows(got), key=repr) == sorted(rows_of(want, ["s", "n", "m"]), key=repr)


@pytest.mark.gpu
def test_a_retained_cross_join_feeds_the_next_stage_from_the_device(gpu):
    from flock_amd.runtime import ExecutionContext
    nl, nr = 9, 1031
    left, right = make_table(nl, 71, 0.2), make_table(nr, 73, 0.2, "_r")
    both = COLS + RCOLS
    producer = ExecutionContext([_cross(_scan(COLS), _scan(RCOLS), COLS, RCOLS)], gpu=gpu)
    keep = [("s2", "Utf8"), ("f_r", "Float64"), ("u", "UInt64")]
    consumer = ExecutionContext([_project(_scan(both), [(_c(c, both), c) for c, _ in keep], keep)], gpu=gpu)
    try:
        producer.feed_data_sources([[_batches(left, 4, COLS)], [_batches(right, 500, RCOLS)]])
        assert producer.execute_retain() == [nl * nr]
        consumer.feed_from([producer])
        out = consumer.execute()[0][0]
    finally:
        consumer.close()
        producer.close()
    xt = cross_table(left, right)
    assert _pyrows(out) == _norm(rows_of(xt, [c for c, _ in keep]))


# ------------------------------------------------------------------ GPU 6: limits and the one-row path
@pytest.mark.gpu
def test_two_to_the_31_rows_are_refused_before_anything_runs(gpu):
    """46 341 x 46 341 = 2 147 488 281 >= 2^31 row COUNTS through two single-column tables: an argument check, nothing is produced; the context runs the
    next plan afterwards."""
    from flock_amd import _ffi
    from flock_amd.runtime import ExecutionContext, FlockGpuError, collect
    n = 46_341
    lc, rc = [("k", "Int32")], [("k_r", "Int32")]
    one = np.arange(n, dtype=np.int32)
    ctx = ExecutionContext([_cross(_scan(lc), _scan(rc), lc, rc)], gpu=gpu)
    try:
        with pytest.raises(FlockGpuError) as e:
            collect(ctx, [[[pa.record_batch([pa.array(one)], names=["k"])]], [[pa.record_batch([pa.array(one)], names=["k_r"])]]])
        assert e.value.code == _ffi.ERR_UNSUPPORTED, str(e.value)
        assert "cross join" in str(e.value) and str(e.value).count("46341") == 2 and "2^31 rows" in str(e.value), str(e.value)
    finally:
        ctx.close()
    _check_cross(gpu, make_table(3, 1), make_table(4, 2, 0.0, "_r"))


@pytest.mark.gpu
def test_a_utf8_column_of_two_to_the_31_bytes_is_refused(gpu):
    """3 x 1100 rows of one 700 000-byte string on the left: 2.31e9 bytes of output for that column, 3300 rows"""
    from flock_amd import _ffi
    from flock_amd.runtime import ExecutionContext, FlockGpuError, collect
    lc, rc = [("big", "Utf8")], [("k_r", "Int32")]
    ctx = ExecutionContext([_cross(_scan(lc), _scan(rc), lc, rc)], gpu=gpu)
    try:
        with pytest.raises(FlockGpuError) as e:
            collect(ctx, [[[pa.record_batch([pa.array(["q" * 700_000] * 3)], names=["big"])]], [[pa.record_batch([pa.array(np.arange(1100, dtype=np.int32))], names=["k_r"])]]])
        assert e.value.code == _ffi.ERR_UNSUPPORTED and "exceeds 2^31 bytes" in str(e.value) and "big" in str(e.value), str(e.value)
    finally:
        ctx.close()
    _check_cross(gpu, make_table(2, 3), make_table(2, 4, 0.0, "_r"))


@pytest.mark.gpu
@pytest.mark.parametrize("one_on_the_right", [True, False])
def test_one_row_costs_fills_and_nothing_per_column_of_the_other_side(gpu, one_on_the_right):
    """bid CROSS JOIN (one row) with every bid column required: no cross_tile / cross_repeat launch -- the bid columns are the bid table's own --,
    only the fills of the one row's columns."""
    from flock_amd.runtime import ExecutionContext, collect
    n = ROWS4 * 2 + 77
    bid = _bids(n, 79)
    acols = [("p_r", "Int32")]
    entries = [_entry("max", "MAX(p_r)", "Int32", _c("p_r", acols)), _entry("avg", "AVG(p_r)", "Float64", _c("p_r", acols))]
    rcols = [("MAX(p_r)", "Int32"), ("AVG(p_r)", "Float64")]
    row = _ungrouped(entries, _scan(acols), acols)
    plan = _cross(_scan(BID), row, BID, rcols) if one_on_the_right else _cross(row, _scan(BID), rcols, BID)
    feeds = [[_batches(bid, 4096, BID)], [_batches({"p_r": bid["price"]}, 4096, acols)]]
    ctx = ExecutionContext([plan], gpu=gpu)
    gpu.profile_reset()
    gpu.profile(True)
    try:
        out = collect(ctx, feeds if one_on_the_right else feeds[::-1])[0][0]
        ran = gpu.profile_read()
    finally:
        gpu.profile(False)
        ctx.close()
    one = [(max(bid["price"]), sum(bid["price"]) / n)]
    brows = rows_of(bid, [c for c, _ in BID])
    assert _pyrows(out) == _norm(cross_rows(brows, one) if one_on_the_right else cross_rows(one, brows))
    assert "cross_fill_kernel" in ran, sorted(ran)
    for k in ran:
        assert not any(w in k for w in ("cross_tile", "cross_repeat", "gather", "take")), sorted(ran)
