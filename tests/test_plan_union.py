"""UnionExec (union.hpp A-U1..7): UNION ALL -- the rows of input 0 in their order, then input 1's, and so on -- against the plain-Python reference of
tests/union_ref.py, row for row IN ORDER, validity included (floats by their bits)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pyarrow as pa
import pytest

from union_ref import check_limits, rows_of, union_count, union_rows, union_schema, union_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")


def _header_int(name):
    text = open(os.path.join(ROOT, "flock_amd", "csrc", "union.hpp")).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))


CHUNKS = _header_int("kUnionTileChunks")     # 16-byte output chunks of one workgroup
ROWS4 = CHUNKS * 4                           # rows of one workgroup of the 4-byte kernel (8-byte: half, validity bytes: four times as many)
SOURCES = _header_int("kUnionSources")       # sources of one launch
MAX_INPUTS = _header_int("kUnionMaxInputs")

_TS = {"Timestamp": ["Millisecond", None]}
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string(), "ts": pa.timestamp("ms")}
COLS = [("i", "Int32"), ("l", "Int64"), ("u", "UInt64"), ("t", "ts"), ("f", "Float64"), ("s", "Utf8")]
NAMES = [c for c, _ in COLS]
WORDS = ["", "a", "b" * 15, "c" * 16, "d" * 17, "é" * 35]     # 0, 1, 15, 16, 17 and 70 bytes
FLOATS = [float("inf"), float("-inf"), -0.0, 0.0, 1.5, -2.25e300, 4.9e-324]


# ------------------------------------------------------------------ plans
def _dt(t):
    return _TS if t == "ts" else t


def _field(name, t, nullable=True):
    return {"data_type": _dt(t), "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


def _schema(cols):
    return {"fields": [_field(n, t) for n, t in cols], "metadata": {}}


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


def _coalesce(inp):
    return {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096, "input": inp}


def _filter(inp, pred):
    return _coalesce({"execution_plan": "filter_exec", "predicate": pred, "input": inp})


def _project(inp, exprs, cols):
    return {"execution_plan": "projection_exec", "expr": [[e, n] for e, n in exprs], "input": inp, "schema": _schema(cols)}


def _union(inputs, cols=None):
    p = {"execution_plan": "union_exec", "inputs": inputs}
    if cols is not None:
        p["schema"] = _schema(cols)
    return p


def _count_star():
    return {"aggregate_expr": "count", "name": "COUNT(UInt8(1))", "data_type": "UInt64", "nullable": True, "expr": _lit("UInt8", 1)}


def _entry(fn, name, ty, expr):
    return {"aggregate_expr": fn, "name": name, "data_type": _dt(ty), "nullable": True, "expr": expr}


def _agg(mode, group, entries, inp, in_cols, out_cols):
    return {"execution_plan": "hash_aggregate_exec", "mode": mode, "group_expr": group, "aggr_expr": entries, "input": inp, "input_schema": _schema(in_cols),
            "schema": _schema(out_cols)}


def _ungrouped(entries, inp, in_cols):
    """Partial -> CoalescePartitions -> Final, as the planner writes SELECT <aggregates> FROM ..."""
    part = _agg("Partial", [], entries, inp, in_cols, [("%s[%s]" % (e["name"], e["aggregate_expr"]), e["data_type"]) for e in entries])
    return _agg("Final", [], entries, {"execution_plan": "coalesce_partitions_exec", "input": part}, in_cols, [(e["name"], e["data_type"]) for e in entries])


def _hashp(inp, names, parts=4):
    return {"execution_plan": "repartition_exec", "input": inp,
            "partitioning": {"Hash": [[{"physical_expr": "column", "name": n, "index": i} for i, n in enumerate(names)], parts]}}


def _grouped(keys, entries, inp, in_cols):
    """Partial -> Repartition Hash(keys) -> FinalPartitioned over the key columns `keys` [(name, type)] of `inp`"""
    state = [("%s[%s]" % (e["name"], e["aggregate_expr"]), e["data_type"]) for e in entries]
    part = _agg("Partial", [[_c(k, in_cols), k] for k, _ in keys], entries, inp, in_cols, keys + state)
    return _agg("FinalPartitioned", [[{"physical_expr": "column", "name": k, "index": i}, k] for i, (k, _) in enumerate(keys)], entries,
                _coalesce(_hashp(part, [k for k, _ in keys])), in_cols, keys + [(e["name"], e["data_type"]) for e in entries])


def _sfx(cols, k):
    return [("%s_%d" % (c, k) if k else c, t) for c, t in cols]


# ------------------------------------------------------------------ tables: {name: list of Python values, None = NULL}
def _words(n, seed):
    """n values over every length of WORDS whose byte total is ODD (n >= 1): the next input's bytes begin at an odd address"""
    w = [WORDS[(seed + k * 5) % len(WORDS)] for k in range(n)]
    if n and sum(len(x.encode()) for x in w) % 2 == 0:
        w[0] = "a" if len(w[0].encode()) % 2 == 0 else ""
    return w


def make_table(n, seed, null_p=0.0, k=0):
    r = np.random.default_rng(seed)
    t = {"i": [int(x) for x in r.permutation(4 * n + 3)[:n] * 1000 - 2**20 + seed],              # unique per row
         "l": [int(x) for x in r.integers(-2**62, 2**62, n)],
         "u": [2**63 + int(x) for x in r.integers(0, 2**62, n)],
         "t": [1_436_918_400_000 + int(x) for x in r.integers(0, 10**9, n)],
         "f": [FLOATS[j % len(FLOATS)] if j % 3 else float(np.round(r.normal(0, 1e6), 3)) for j in range(n)],
         "s": _words(n, seed)}
    if null_p > 0:
        for c in NAMES:
            m = r.random(n) < null_p
            t[c] = [None if m[j] else t[c][j] for j in range(n)]
    return {("%s_%d" % (c, k) if k else c): v for c, v in t.items()}


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
    """feeds: one list of batches per SOURCE, in the order the leaves take them; the one output batch (of the last execute)"""
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        for _ in range(executes):
            out = collect(ctx, [[f] for f in feeds])[0]
    finally:
        ctx.close()
    assert len(out) == 1
    return out[0]


def _tables(shape, seed, nulls):
    """one table per input; `nulls`: validity in the ODD inputs only"""
    return [make_table(n, seed + 7 * k, 0.3 if nulls and k % 2 else 0.0, k) for k, n in enumerate(shape)]


def _check_union(gpu, shape, seed, nulls, chunk=1500):
    tabs = _tables(shape, seed, nulls)
    plan = _union([_scan(_sfx(COLS, k)) for k in range(len(shape))])
    out = _run(gpu, plan, [_batches(t, chunk, _sfx(COLS, k)) for k, t in enumerate(tabs)])
    assert out.schema.names == NAMES                                              # A-U1: input 0's names
    want = _norm(union_rows([rows_of(t, [c for c, _ in _sfx(COLS, k)]) for k, t in enumerate(tabs)]))
    got = _pyrows(out)
    assert len(got) == len(want) == sum(shape)
    assert got == want
    return out


# ------------------------------------------------------------------ CPU: the reference itself
def test_reference_on_hand_worked_rows_and_against_pyarrow():
    a, b, c = [(1, "x"), (None, "y")], [], [(3, None), (1, "x")]
    assert union_rows([a, b, c]) == [(1, "x"), (None, "y"), (3, None), (1, "x")]                  # A-U2, A-U3: in order, NULLs and duplicates verbatim
    assert union_rows([b, b]) == [] and union_rows([a]) == a                                     # A-U4, one input
    assert union_rows([a, c], keep=[1]) == [("x",), ("y",), (None,), ("x",)] and union_rows([a, c], keep=[]) == [()] * 4 and union_count([a, b, c]) == 4
    assert union_table([{"p": [1, 2], "q": ["a", None]}, {"x": [3], "y": ["b"]}]) == {"p": [1, 2, 3], "q": ["a", None, "b"]}     # by position, input 0's names
    assert union_schema([[("p", "Int32", False)], [("x", "Int32", True)]]) == [("p", "Int32", True)]                             # nullable in any input
    for bad, words in (([[("p", "Int32", False)], [("p", "Int64", False)]], ("input 1", "'p'", "Int64", "Int32")),
                       ([[("p", "Int32", False)], [("p", "Int32", False), ("q", "Utf8", True)]], ("input 1", "2 columns", "has 1")), ([], ("no inputs",))):
        with pytest.raises(ValueError) as e:
            union_schema(bad)
        assert all(w in str(e.value) for w in words), str(e.value)
    check_limits([2**31 - 2, 1], [2**31 - 1])
    for rows, bytes_ in (([2**31 - 1, 1], []), ([2**30] * 2, []), ([1], [2**30, 2**30])):
        with pytest.raises(ValueError):
            check_limits(rows, bytes_)
    # pyarrow's own concatenation, column by column, over tables of every type with NULLs
    tabs = [make_table(n, 3 + n, 0.3) for n in (5, 0, 7, 1)]
    pat = pa.concat_tables([pa.table({c: pa.array(t[c], _PA[ty]) for c, ty in COLS}) for t in tabs])
    ours = union_table(tabs)
    for c, ty in COLS:
        col = pat.column(c).cast(pa.int64()) if ty == "ts" else pat.column(c)
        assert _norm([(v,) for v in col.to_pylist()]) == _norm([(v,) for v in ours[c]])
    assert pat.num_rows == union_count([rows_of(t, NAMES) for t in tabs]) == 13


def test_host_index_helpers_under_the_sanitizers():
    """union.hpp's host-callable helpers (the source of an element, a seam's position in a chunk, rebased offsets, the A-U6 checks -- 2^31 rows and
    bytes as COUNTS, nothing is allocated) in a stand-alone program built with AddressSanitizer and UBSan: host code on the CPU."""
    import subprocess
    exe = os.path.join(ROOT, "tests", "cpp", "union_index_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "flock_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "union_index_test.cpp"), "-o", exe])
    assert "union_index_test ok" in subprocess.check_output([exe], text=True)


# ------------------------------------------------------------------ CPU: parsing, refusals, recognition, pruning, stage split
def _head(line):
    return [x.split(":") for x in line[line.index("[") + 1:line.index("]")].split(", ")]


def test_explain_for_one_two_nested_and_seventeen_inputs():
    from flock_amd.runtime import explain
    one = explain(_union([_scan(COLS)])).splitlines()
    assert one[0].startswith("Union(1 inputs) [") and len(one) == 2 and one[1].strip().startswith("Scan"), one
    assert [n for n, _ in _head(one[0])] == NAMES and [t for _, t in _head(one[0])] == ["Int32", "Int64", "UInt64", "Timestamp(ms)", "Float64", "Utf8"]
    two = explain(_union([_scan(COLS), _scan(_sfx(COLS, 1))], COLS)).splitlines()
    assert two[0].startswith("Union(2 inputs) [") and len(two) == 3 and [n for n, _ in _head(two[0])] == NAMES, two            # names from input 0
    assert explain(_union([_scan(COLS), _scan(_sfx(COLS, 1))])).splitlines()[0] == two[0]                                       # the node's schema is optional
    # a union directly under a union -- also through the transparent nodes and a round-robin repartition -- gives its inputs to the outer one, in order
    rr = {"execution_plan": "repartition_exec", "partitioning": {"RoundRobinBatch": 8}, "input": _union([_scan(_sfx(COLS, 3)), _scan(_sfx(COLS, 4))])}
    inner = _coalesce({"execution_plan": "coalesce_partitions_exec", "input": _union([_scan(_sfx(COLS, 1)), _scan(_sfx(COLS, 2))])})
    nested = explain(_union([_scan(COLS), inner, rr])).splitlines()
    assert nested[0].startswith("Union(5 inputs) [") and len(nested) == 6, nested
    assert [_head(ln)[0][0] for ln in nested[1:]] == ["i", "i_1", "i_2", "i_3", "i_4"] and all(ln.startswith("  Scan") for ln in nested[1:])
    # ... but not through a filter: that union stays a node of its own
    kept = explain(_union([_scan(COLS), _filter(_union([_scan(_sfx(COLS, 1)), _scan(_sfx(COLS, 2))]), _bin(_c("i_1", _sfx(COLS, 1)), "Gt", _lit("Int32", 0)))]))
    assert kept.count("Union(2 inputs)") == 2, kept
    many = explain(_union([_scan(_sfx(COLS, k)) for k in range(17)])).splitlines()
    assert many[0].startswith("Union(17 inputs) [") and len(many) == 18
    assert explain(_union([_scan(_sfx(COLS, k)) for k in range(MAX_INPUTS)])).startswith("Union(%d inputs)" % MAX_INPUTS)


def _refused(plan, *words):
    from flock_amd import _ffi
    from flock_amd.runtime import FlockGpuError, explain
    with pytest.raises(FlockGpuError) as e:
        explain(plan)
    assert e.value.code in (_ffi.ERR_UNSUPPORTED, _ffi.ERR_PLAN), str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals_by_name():
    other = [("i_1", "Int32"), ("l_1", "Int32")] + _sfx(COLS, 1)[2:]                        # l: Int64 in input 0
    _refused(_union([_scan(COLS), _scan(COLS), _scan(other)]), "Union", "input 2", "column 1", "'l_1'", "Int32", "Int64")
    stamp = [("i_1", "Int32"), ("l_1", "Int64"), ("u_1", "UInt64"), ("t_1", "Int64")] + _sfx(COLS, 1)[4:]     # t: a Timestamp in input 0 (the same storage)
    _refused(_union([_scan(COLS), _scan(stamp)]), "Union", "input 1", "column 3", "Timestamp(ms)", "Int64")
    _refused(_union([_scan(COLS), _scan(_sfx(COLS, 1)[:-1])]), "Union", "input 1", "5 columns", "input 0 has 6")
    _refused(_union([]), "Union", "no inputs")
    _refused({"execution_plan": "union_exec"}, "Union", "no inputs")
    _refused(_union([_scan(_sfx(COLS, k)) for k in range(MAX_INPUTS + 1)]), "Union", "more than %d inputs" % MAX_INPUTS)
    # ... counted AFTER flattening: 33 + 32 inputs
    _refused(_union([_union([_scan(_sfx(COLS, k)) for k in range(33)]), _union([_scan(_sfx(COLS, k)) for k in range(32)])]), "Union", "more than %d inputs" % MAX_INPUTS)
    short = _union([_scan(COLS), _scan(_sfx(COLS, 1))], COLS[:-1])
    _refused(short, "Union", "schema", "5 columns", "6 columns")
    wrong = _union([_scan(COLS), _scan(_sfx(COLS, 1))], [("i", "Int32"), ("l", "Float64")] + COLS[2:])
    _refused(wrong, "Union", "schema", "'l'", "Float64", "Int64")
    _refused(_union([_scan(COLS), {"execution_plan": "no_such_exec"}]), "no_such_exec")


def _scan_reads(text):
    return [ln[ln.index("reads [") + 7:ln.rindex("]")] for ln in text.splitlines() if ln.strip().startswith("Scan")]


def test_pruning_reaches_every_leaf_and_leaves_of_one_relation_share_their_columns():
    """A-U5: COUNT(*) over a union asks no leaf for a column; a projection of two columns asks every leaf for its two.  A-U7: two branches over the SAME
    field list upload the columns either of them reads -- only in a plan with a union."""
    from flock_amd.runtime import explain
    u = _union([_scan(_sfx(COLS, k)) for k in range(3)])
    assert _scan_reads(explain(u)) == [", ".join(c for c, _ in _sfx(COLS, k)) for k in range(3)]
    assert _scan_reads(explain(_ungrouped([_count_star()], u, COLS))) == ["", "", ""]
    two = _project(u, [(_c("s", COLS), "s"), (_c("l", COLS), "l")], [("s", "Utf8"), ("l", "Int64")])
    assert _scan_reads(explain(two)) == ["l, s", "l_1, s_1", "l_2, s_2"]
    text = explain(open(os.path.join(PLANS, "bids_two_ranges.json")).read())
    assert _scan_reads(text) == ["auction, bidder, price, b_date_time"] * 2, text
    # the same two branches as the sides of a cross join: every leaf reads its own branch's columns, as it always did
    p = json.load(open(os.path.join(PLANS, "bids_two_ranges.json")))
    x = {"execution_plan": "cross_join_exec", "left": p["inputs"][0], "right": p["inputs"][1]}
    assert _scan_reads(explain(x)) == ["auction, price", "bidder, b_date_time"]


def test_the_fixtures_explain_and_no_plan_with_a_union_is_a_fused_query():
    from flock_amd import _ffi, build
    from flock_amd.runtime import explain
    build.build()
    lib = _ffi.load()
    got = C.c_int(-1)

    def recognised(plan):
        raw = (plan if isinstance(plan, str) else json.dumps(plan)).encode()
        assert lib.flockgpu_plan_recognise(raw, len(raw), C.byref(got)) == _ffi.OK
        return got.value
    act = open(os.path.join(PLANS, "person_activity.json")).read()
    lines = explain(act).splitlines()
    assert lines[0].startswith("Aggregate(FinalPartitioned) [person:Int32, kind:Utf8, COUNT(UInt8(1)):UInt64]")
    assert lines[3].strip().startswith("Union(2 inputs) [person:Int32, t:Timestamp(ms), kind:Utf8]"), lines
    assert _scan_reads(explain(act)) == ["seller", "bidder"]
    assert recognised(act) == 0 and recognised(open(os.path.join(PLANS, "bids_two_ranges.json")).read()) == 0
    # a fused sub-tree stays fused below a union; the plan as a whole is no NEXMark query
    q2 = json.load(open(os.path.join(PLANS, "q2.json")))
    assert recognised(q2) == 2
    alone = explain(q2)
    marks = [ln.split("<- ")[1] for ln in alone.splitlines() if "<- " in ln and "generic" not in ln]
    assert marks, alone
    both = explain(_union([q2, q2]))
    assert recognised(_union([q2, q2])) == 0 and recognised(_union([q2])) == 0
    assert [ln.split("<- ")[1] for ln in both.splitlines() if "<- " in ln and "generic" not in ln] == marks * 2, both


def test_the_stage_splitter_walks_a_unions_inputs_and_does_not_cut_at_it():
    from flock_amd.runtime import explain
    from flock_amd.stages import build_query_dag, leaves_bfs, node_schema, split_at_repartitions
    act = json.load(open(os.path.join(PLANS, "person_activity.json")))
    stages = build_query_dag(act)
    assert len(stages) == 2 and [st.is_shuffling for st in stages] == [True, False]
    assert stages[0].inputs == [None, None] and stages[1].inputs == [0]
    low = explain(stages[0].plan)
    assert "Union(2 inputs)" in low and low.count("Scan") == 2 and "Aggregate(Partial)" in low and "Union" not in explain(stages[1].plan)
    # the schema of a union: its own, else input 0's
    u = _union([_scan(_sfx(COLS, 1)), _scan(_sfx(COLS, 2))])
    assert [f["name"] for f in node_schema(u)["fields"]] == [c for c, _ in _sfx(COLS, 1)]
    assert [f["name"] for f in node_schema(_union(u["inputs"], COLS))["fields"]] == NAMES
    assert [f["name"] for lf in leaves_bfs(_union([u, _scan(COLS)])) for f in lf["schema"]["fields"][:1]] == ["i", "i_1", "i_2"]      # breadth first
    # a sort over a union: one cut, the lower stage is the union with both scans
    sort = {"execution_plan": "sort_exec", "input": u, "expr": [{"expr": _c("i_1", _sfx(COLS, 1)), "options": {"descending": False, "nulls_first": False}}]}
    st = build_query_dag(sort)
    assert len(st) == 2 and explain(st[0].plan).startswith("Union(2 inputs)") and st[0].inputs == [None, None] and st[1].inputs == [0]
    # repartitions INSIDE the branches: each becomes a shuffling stage of its own, the union keeps a leaf in its place
    b0 = _coalesce(_hashp(_scan(COLS), ["i"]))
    b1 = _filter(_coalesce(_hashp(_scan(_sfx(COLS, 1)), ["i_1"])), _bin(_c("i_1", _sfx(COLS, 1)), "Gt", _lit("Int32", 0)))
    top = _ungrouped([_count_star()], _union([b0, b1, _scan(_sfx(COLS, 2))]), COLS)
    parts = split_at_repartitions(top)
    # (the gather under the Final aggregate is a cut of its own: the Partial aggregate over the union runs below it)
    assert len(parts) == 4 and [p.is_shuffling for p in parts] == [True, True, False, False], [p.plan for p in parts]
    assert parts[2].inputs == [0, None, 1] and parts[0].inputs == [None] and parts[1].inputs == [None] and parts[3].inputs == [2]
    mid = explain(parts[2].plan)                                   # (leaves breadth-first: the filter's leaf lies deeper than the plain scan)
    assert "Union(3 inputs)" in mid and mid.count("Scan") == 3 and "Repartition" not in mid and "Filter" in mid
    assert top["input"]["input"]["input"]["inputs"][0] is b0                                      # (the caller's plan is left as it was)


# ------------------------------------------------------------------ GPU 1: shapes
# Input row counts from {0, 1, 3, 5, 7, 4097}: the seams fall at every misalignment mod 16 bytes for the widths 1, 4 and 8 (prefix sums 1, 3, 5, 7, 9, 11,
# 13, 15 ... and their doubles), (5, 4097, ..) puts a seam inside the first workgroup's tile, (4097, ..) one in the FIRST chunk of the second
# workgroup's (row 4097 of a 4-byte column lies in chunk 1024) and (4097, 4097, 4097, 4097, 3) carries the validity bytes past their first tile too.
SHAPES = [(5,), (1, 1), (1, 3, 5, 7), (7, 5, 3, 1, 1, 3), (0, 5, 0, 7, 0), (3, 7, 3, 7, 1, 5, 5), (5, 4097, 3), (4097, 7, 1), (4097, 4097, 4097, 4097, 3),
          (0, 0, 0), (1, 3, 5, 7, 1, 3, 5, 7, 0, 1, 3, 5, 7, 1, 3, 5, 7), tuple([1, 3, 5, 7] * 8 + [4097])]


@pytest.mark.gpu
@pytest.mark.parametrize("nulls", [False, True], ids=["plain", "nulls"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)) if len(s) < 8 else "%d_inputs" % len(s))
def test_every_row_in_input_order(gpu, shape, nulls):
    """one input; seams at every misalignment; empty inputs between others; every input empty (A-U4); 17 inputs (two rounds of sources) and 33 (three);
    `nulls`: validity bytes in the odd inputs only (A-U3)"""
    assert len(SHAPES[-2]) == SOURCES + 1 and len(SHAPES[-1]) == 2 * SOURCES + 1
    out = _check_union(gpu, shape, 11 + len(shape), nulls)
    for c in out.columns:
        assert c.null_count == 0 or nulls, (shape, c.null_count)
        assert c.null_count > 0 or not nulls or sum(shape[1::2]) < 100, (shape, c.null_count)


@pytest.mark.gpu
def test_utf8_byte_seams_fall_at_odd_and_even_addresses(gpu):
    """every input's byte total is odd (make_table), so the inputs' bytes begin at alternating parities; single-value inputs of every length put a seam
    at every distance from a 16-byte boundary"""
    tabs = [{"s_%d" % k if k else "s": [w]} for k, w in enumerate(WORDS[1:] * 3 + ["", "", "x"] + WORDS[::-1])]
    cols = lambda k: [("s_%d" % k if k else "s", "Utf8")]
    out = _run(gpu, _union([_scan(cols(k)) for k in range(len(tabs))]), [_batches(t, 8, cols(k)) for k, t in enumerate(tabs)])
    assert out.column(0).to_pylist() == [w for t in tabs for w in list(t.values())[0]]
    for n in (1, 3, 5, 7, 4097):
        assert sum(len(w.encode()) for w in _words(n, n)) % 2 == 1


@pytest.mark.gpu
def test_batching_and_a_second_execute_change_no_byte(gpu):
    from flock_amd.runtime import ExecutionContext, collect
    shape = (23, 0, 19, 7)
    tabs = _tables(shape, 5, True)
    plan = _union([_scan(_sfx(COLS, k)) for k in range(len(shape))])
    seen = []
    for chunk in (32, 1, 7):
        ctx = ExecutionContext([plan], gpu=gpu)
        try:
            for _ in range(2):                       # (the second execute finds the first one's arenas)
                out = collect(ctx, [[_batches(t, chunk, _sfx(COLS, k))] for k, t in enumerate(tabs)])[0]
                assert len(out) == 1
                seen.append((_buffers(out[0]), _pyrows(out[0])))
        finally:
            ctx.close()
    assert all(s[1] == seen[0][1] for s in seen)
    assert all(s[0] == seen[0][0] for s in seen)
    assert seen[0][1] == _norm(union_rows([rows_of(t, [c for c, _ in _sfx(COLS, k)]) for k, t in enumerate(tabs)]))


# ------------------------------------------------------------------ GPU 2: row lists, all_null columns, the one-input path
def _pred(which, cols, k):
    """selectivity 0, ~1/3 and 1 over the unique Int32 column; a NULL there fails every one of them"""
    i = _c("i_%d" % k if k else "i", cols)
    if which == "none":
        return _bin(i, "Lt", _lit("Int32", -2**31))
    if which == "third":
        return _bin(_bin(_cast(i, "Int64"), "Modulo", _lit("Int64", 3)), "Eq", _lit("Int64", 0))
    return _bin(i, "GtEq", _lit("Int32", -2**31))


def _keep(t, which, k):
    col = t["i_%d" % k if k else "i"]
    return [v is not None and (which == "all" or (which == "third" and v % 3 == 0)) for v in col]


@pytest.mark.gpu
@pytest.mark.parametrize("which", [("third", None, "third", "all"), (None, "third", "none", None, "third"), ("none", "none"), ("third",), ("all", "none", None)],
                         ids=lambda w: "-".join(x or "plain" for x in w))
def test_filters_directly_under_the_union_beside_plain_inputs(gpu, which):
    """row lists for fixed-width values, validity bytes (inputs 1 and 3 hold NULLs) and Utf8 columns, beside plain inputs in the same union; a lone input
    with a row list; filters that keep nothing"""
    shape = (211, 157, 4097, 64, 33)[:len(which)]
    tabs = [make_table(n, 31 + k, 0.25 if k % 2 else 0.0, k) for k, n in enumerate(shape)]
    ins = [_scan(_sfx(COLS, k)) if w is None else _filter(_scan(_sfx(COLS, k)), _pred(w, _sfx(COLS, k), k)) for k, w in enumerate(which)]
    out = _run(gpu, _union(ins), [_batches(t, 1000, _sfx(COLS, k)) for k, t in enumerate(tabs)], executes=2)
    want = []
    for k, (t, w) in enumerate(zip(tabs, which)):
        rows = rows_of(t, [c for c, _ in _sfx(COLS, k)])
        want.append(rows if w is None else [r for r, kept in zip(rows, _keep(t, w, k)) if kept])
    if which[0] == "third":
        assert shape[0] // 6 < len(want[0]) < shape[0] // 2
    assert _pyrows(out) == _norm(union_rows(want)) and out.num_rows == sum(len(w) for w in want)


def _max_over(cols):
    return _ungrouped([_entry("max", "MAX(%s)" % cols[0][0], "Int32", _c(cols[0][0], cols))], _scan(cols), cols)


@pytest.mark.gpu
def test_all_null_columns_of_one_input_and_of_every_input(gpu):
    """MAX over no rows is one row whose column is nothing but NULLs (DevColumn::all_null, no validity bytes).  Beside inputs with values it
    contributes zero validity (A-U3); where every input is such a row the column stays what it is."""
    e1, e2, m = [("p", "Int32")], [("q", "Int32")], [("m", "Int32")]
    empty = lambda name: [pa.record_batch([pa.array([], pa.int32())], names=[name])]
    vals = {"m": [7, None, -3]}
    mixed = _union([_max_over(e1), _scan(m), _max_over(e2)])
    out = _run(gpu, mixed, [empty("p"), _batches(vals, 8, m), empty("q")])
    assert out.schema.names == ["MAX(p)"] and out.column(0).to_pylist() == [None, 7, None, -3, None]
    plain = {"m": [5, 6]}                                                     # an input without validity bytes beside the NULL row: ones
    out = _run(gpu, _union([_scan(m), _max_over(e1)]), [_batches(plain, 8, m), empty("p")])
    assert out.column(0).to_pylist() == [5, 6, None]
    out = _run(gpu, _union([_max_over(e1), _max_over(e2)]), [empty("p"), empty("q")])
    assert out.column(0).to_pylist() == [None, None] and out.num_rows == 2
    # ... and a MAX that found a row, beside one that found none
    out = _run(gpu, _union([_max_over(e1), _max_over(e2)]), [_batches({"p": [4, 9, 2]}, 8, e1), empty("q")])
    assert out.column(0).to_pylist() == [9, None]


@pytest.mark.gpu
def test_one_plain_input_with_rows_is_the_result_itself(gpu):
    """exactly one input has rows and it is a plain table: its columns ARE the result -- no union kernel is launched; with a second non-empty input the
    union's kernels show in the profile"""
    from flock_amd.runtime import ExecutionContext, collect
    t0, t1 = make_table(ROWS4 + 5, 91, 0.2), make_table(0, 92, 0.0, 1)
    plan = _union([_scan(COLS), _scan(_sfx(COLS, 1)), _filter(_scan(_sfx(COLS, 2)), _pred("none", _sfx(COLS, 2), 2))])
    feeds = [[_batches(t0, 4096, COLS)], [_batches(t1, 8, _sfx(COLS, 1))], [_batches(make_table(9, 93, 0.0, 2), 8, _sfx(COLS, 2))]]
    ran = []
    for second in (t1, make_table(3, 94, 0.0, 1)):
        feeds[1] = [_batches(second, 8, _sfx(COLS, 1))]
        ctx = ExecutionContext([plan], gpu=gpu)
        gpu.profile_reset()
        gpu.profile(True)
        try:
            out = collect(ctx, feeds)[0][0]
            ran.append(gpu.profile_read())
        finally:
            gpu.profile(False)
            ctx.close()
        assert _pyrows(out) == _norm(union_rows([rows_of(t0, NAMES), rows_of(second, [c for c, _ in _sfx(COLS, 1)])]))
    assert not [k for k in ran[0] if k.startswith("union_")], ran[0]
    assert {"union_fixed_kernel", "union_valid_kernel", "union_offsets_kernel", "union_bytes_kernel"} <= set(ran[1]), ran[1]


# ------------------------------------------------------------------ GPU 3: positions in a plan
K3 = [("k", "Int32"), ("v", "Int64"), ("s", "Utf8")]
D = [("d", "Int32"), ("df", "Float64")]


def _k3(n, seed, k, null_p=0.0):
    r = np.random.default_rng(seed)
    t = {"k": [int(x) for x in r.integers(0, 12, n)], "v": [int(x) for x in r.integers(-10**12, 10**12, n)], "s": [WORDS[int(x)] for x in r.integers(0, len(WORDS), n)]}
    if null_p:
        for c in ("v", "s"):
            m = r.random(n) < null_p
            t[c] = [None if m[j] else t[c][j] for j in range(n)]
    return {("%s_%d" % (c, k) if k else c): v for c, v in t.items()}


def _three():
    tabs = [_k3(40, 1, 0), _k3(0, 2, 1), _k3(ROWS4 + 9, 3, 2, 0.2)]
    plan = _union([_scan(_sfx(K3, k)) for k in range(3)])
    feeds = [_batches(t, 2048, _sfx(K3, k)) for k, t in enumerate(tabs)]
    rows = union_rows([rows_of(t, [c for c, _ in _sfx(K3, k)]) for k, t in enumerate(tabs)])
    return plan, feeds, rows


@pytest.mark.gpu
def test_under_count_star_group_by_filter_and_sort_limit(gpu):
    u, feeds, rows = _three()
    # COUNT(*) reads no column (A-U5): the sum of the inputs' row counts
    assert _run(gpu, _ungrouped([_count_star()], u, K3), feeds).column(0).to_pylist() == [len(rows)]
    # SUM(v), COUNT(v): the NULLs of input 2 are skipped
    out = _run(gpu, _ungrouped([_entry("sum", "SUM(v)", "Int64", _c("v", K3)), _entry("count", "COUNT(v)", "UInt64", _c("v", K3))], u, K3), feeds)
    assert [c.to_pylist()[0] for c in out.columns] == [sum(r[1] for r in rows if r[1] is not None), sum(r[1] is not None for r in rows)]
    # GROUP BY k, s: COUNT(*), MAX(v) -- the groups straddle the inputs
    got = _run(gpu, _grouped([("k", "Int32"), ("s", "Utf8")], [_count_star(), _entry("max", "MAX(v)", "Int64", _c("v", K3))], u, K3), feeds)
    want = {}
    for k, v, s in rows:
        n, mx = want.get((k, s), (0, None))
        want[(k, s)] = (n + 1, mx if v is None else v if mx is None else max(mx, v))
    assert sorted(_pyrows(got), key=repr) == sorted([(k, s, n, mx) for (k, s), (n, mx) in want.items()], key=repr)
    # a filter over the union keeps the order
    out = _run(gpu, _filter(u, _bin(_c("k", K3), "Lt", _lit("Int32", 4))), feeds)
    assert _pyrows(out) == [r for r in rows if r[0] < 4]
    # ORDER BY v DESC LIMIT 25 (v unique among the valid ones: checked)
    valid = [r for r in rows if r[1] is not None]
    assert len({r[1] for r in valid}) == len(valid)
    sort = {"execution_plan": "sort_exec", "input": _filter(u, {"physical_expr": "is_not_null_expr", "expr": _c("v", K3)}),
            "expr": [{"expr": _c("v", K3), "options": {"descending": True, "nulls_first": False}}]}
    out = _run(gpu, {"execution_plan": "global_limit_exec", "input": sort, "limit": 25}, feeds)
    assert _pyrows(out) == sorted(valid, key=lambda r: -r[1])[:25]


@pytest.mark.gpu
def test_union_distinct_is_a_key_only_aggregate_over_the_union(gpu):
    """SELECT k FROM a UNION SELECT k FROM b: DataFusion plans the DISTINCT as an aggregate without aggregates over the union"""
    u, feeds, rows = _three()
    keys = _project(u, [(_c("k", K3), "k")], [("k", "Int32")])
    out = _run(gpu, _grouped([("k", "Int32")], [], keys, [("k", "Int32")]), feeds)
    assert sorted(out.column(0).to_pylist()) == sorted({r[0] for r in rows}) and out.num_rows == 12


@pytest.mark.gpu
def test_as_a_side_of_a_join_and_of_a_cross_join(gpu):
    u, feeds, rows = _three()
    d = {"d": [1, 2, 3, 1, 40], "df": [0.5, -0.0, None, float("inf"), 2.0]}
    feeds = feeds + [_batches(d, 8, D)]
    drows = rows_of(d, ["d", "df"])
    inner = {"execution_plan": "hash_join_exec", "left": u, "right": _scan(D), "join_type": "Inner", "mode": "CollectLeft", "on": [[_c("k", K3), _c("d", D)]],
             "schema": _schema(K3 + D)}
    got = _pyrows(_run(gpu, inner, feeds))
    assert sorted(got, key=repr) == sorted(_norm(r + q for r in rows for q in drows if r[0] == q[0]), key=repr) and got
    semi = dict(inner, join_type="Semi", schema=_schema(K3))
    assert _pyrows(_run(gpu, semi, feeds)) == [r for r in rows if r[0] in (1, 2, 3)]
    right = dict(inner, left=_scan(D), right=u, on=[[_c("d", D), _c("k", K3)]], schema=_schema(D + K3))
    got = _pyrows(_run(gpu, right, [feeds[3]] + feeds[:3]))
    assert sorted(got, key=repr) == sorted(_norm(q + r for r in rows for q in drows if r[0] == q[0]), key=repr)
    small = _union([_scan(K3), _filter(_scan(_sfx(K3, 1)), _bin(_c("k_1", _sfx(K3, 1)), "Lt", _lit("Int32", 6)))])
    a, b = _k3(5, 7, 0), _k3(9, 8, 1, 0.3)
    urows = union_rows([rows_of(a, ["k", "v", "s"]), [r for r in rows_of(b, ["k_1", "v_1", "s_1"]) if r[0] < 6]])
    x = {"execution_plan": "cross_join_exec", "left": small, "right": _scan(D)}
    assert _pyrows(_run(gpu, x, [_batches(a, 8, K3), _batches(b, 8, _sfx(K3, 1)), _batches(d, 8, D)])) == _norm(r + q for r in urows for q in drows)
    x = {"execution_plan": "cross_join_exec", "left": _scan(D), "right": small}
    assert _pyrows(_run(gpu, x, [_batches(d, 8, D), _batches(a, 8, K3), _batches(b, 8, _sfx(K3, 1))])) == _norm(q + r for q in drows for r in urows)


@pytest.mark.gpu
def test_above_a_join_and_an_aggregate_and_under_another_union(gpu):
    """SELECT k, v FROM a JOIN d ON k = d  UNION ALL  SELECT k_1, MAX(v_1) FROM b GROUP BY k_1  UNION ALL  (SELECT k_2, v_2 FROM c WHERE ..): the inputs'
    own order is the join's / the aggregate's (undefined): each input's SEGMENT of the output is compared as a multiset, the segments in input order"""
    a, b, c = _k3(60, 11, 0), _k3(300, 12, 1, 0.2), _k3(17, 13, 2)
    d = {"d": [1, 2, 3, 1, 40], "df": [0.5, -0.0, None, float("inf"), 2.0]}
    kv = [("k", "Int32"), ("v", "Int64")]
    join = {"execution_plan": "hash_join_exec", "left": _scan(K3), "right": _scan(D), "join_type": "Inner", "mode": "CollectLeft", "on": [[_c("k", K3), _c("d", D)]],
            "schema": _schema(K3 + D)}
    first = _project(join, [(_c("k", K3 + D), "k"), (_c("v", K3 + D), "v")], kv)
    b3 = _sfx(K3, 1)
    second = _grouped([("k_1", "Int32")], [_entry("max", "MAX(v_1)", "Int64", _c("v_1", b3))], _scan(b3), b3)
    c3 = _sfx(K3, 2)
    third = _project(_filter(_scan(c3), _bin(_c("k_2", c3), "GtEq", _lit("Int32", 6))), [(_c("k_2", c3), "k_2"), (_c("v_2", c3), "v_2")], [("k_2", "Int32"), ("v_2", "Int64")])
    plan = _union([first, _union([second, third])])
    out = _run(gpu, plan, [_batches(a, 64, K3), _batches(d, 8, D), _batches(b, 64, b3), _batches(c, 64, c3)])
    w1 = [(k, v) for k, v, _ in rows_of(a, ["k", "v", "s"]) for q in d["d"] if q == k]
    mx = {}
    for k, v, _ in rows_of(b, ["k_1", "v_1", "s_1"]):
        mx[k] = mx.get(k) if v is None else v if mx.get(k) is None else max(mx[k], v)
    w2 = list(mx.items())
    w3 = [(k, v) for k, v, _ in rows_of(c, ["k_2", "v_2", "s_2"]) if k >= 6]
    got = _pyrows(out)
    assert out.schema.names == ["k", "v"] and len(got) == len(w1) + len(w2) + len(w3) and w1 and w3
    assert sorted(got[:len(w1)], key=repr) == sorted(w1, key=repr)
    assert sorted(got[len(w1):len(w1) + len(w2)], key=repr) == sorted(w2, key=repr)
    assert got[len(w1) + len(w2):] == w3


# ------------------------------------------------------------------ GPU 4: the fixtures, one relation in two branches, separate sources
BID = [("auction", "Int32"), ("bidder", "Int32"), ("price", "Int32"), ("b_date_time", "ts")]


def _bids(n, seed):
    r = np.random.default_rng(seed)
    return {"auction": [int(x) for x in r.integers(1000, 2000, n)], "bidder": [int(x) for x in r.integers(0, 500, n)],
            "price": [int(x) for x in r.integers(100, 10_000_000, n)], "b_date_time": [1_436_918_400_000 + 7 * k for k in range(n)]}


@pytest.mark.gpu
def test_the_fixture_person_activity(gpu):
    """the event log over auction and bid under GROUP BY person, kind COUNT(*): two relations, a text literal per branch"""
    r = np.random.default_rng(5)
    na, nb = 700, ROWS4 + 300
    acols = [("a_date_time", "ts"), ("seller", "Int32")]
    auction = {"a_date_time": [1_436_918_400_000 + 11 * k for k in range(na)], "seller": [int(x) for x in r.integers(0, 40, na)]}
    bid = _bids(nb, 6)
    bid["bidder"] = [b % 60 for b in bid["bidder"]]
    plan = open(os.path.join(PLANS, "person_activity.json")).read()
    out = _run(gpu, plan, [_batches(auction, 256, acols), _batches(bid, 1500, BID)], executes=2)
    want = {}
    for p, kind in [(s, "auction") for s in auction["seller"]] + [(b, "bid") for b in bid["bidder"]]:
        want[(p, kind)] = want.get((p, kind), 0) + 1
    assert out.schema.names == ["person", "kind", "COUNT(UInt8(1))"]
    assert sorted(_pyrows(out)) == sorted((p, k, n) for (p, k), n in want.items()) and len(want) == 100


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3000, 12_000])
def test_the_fixture_bids_two_ranges_over_one_fed_source(gpu, n):
    """A-U7: both branches scan `bid`, ONE source is fed -- the first leaf takes it, the second reads the fed one -- and the branches read different
    columns of it (auction, price / bidder, b_date_time): both branches' rows come back, the first branch's first"""
    bid = _bids(n, 17 + n)
    plan = open(os.path.join(PLANS, "bids_two_ranges.json")).read()
    out = _run(gpu, plan, [_batches(bid, 4096, BID)], executes=2)
    high = [a for a, p in zip(bid["auction"], bid["price"]) if p > 9_000_000]
    late = [b for b, t in zip(bid["bidder"], bid["b_date_time"]) if t > 1_436_918_400_000 + 50_000]
    assert out.schema.names == ["id"] and out.column(0).to_pylist() == high + late
    assert (n >= 3000) == bool(high) and (n == 12_000) == bool(late)


@pytest.mark.gpu
def test_two_sources_of_one_schema_reach_one_leaf_each(gpu):
    """two batches of the same relation that arrive as separate sources: the leaves take them in order; with ONE source both leaves read it"""
    b0, b1 = _bids(ROWS4 + 1, 23), _bids(77, 29)
    plan = _union([_scan(BID), _scan(BID)])
    rows = lambda b: rows_of(b, [c for c, _ in BID])
    assert _pyrows(_run(gpu, plan, [_batches(b0, 4096, BID), _batches(b1, 4096, BID)])) == union_rows([rows(b0), rows(b1)])
    assert _pyrows(_run(gpu, plan, [_batches(b1, 4096, BID), _batches(b0, 4096, BID)])) == union_rows([rows(b1), rows(b0)])
    assert _pyrows(_run(gpu, plan, [_batches(b1, 4096, BID)])) == union_rows([rows(b1), rows(b1)])
