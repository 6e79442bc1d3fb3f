"""Random plans over the generic operators against a CPU interpreter: tests/plan_corpus.py draws plans inside the claimed dialect, tests/plan_interp.py
evaluates them row at a time, the GPU tests run them through ExecutionContext + collect -- whole and cut into batches -- and compare EXACTLY: schema
names and Arrow types, rows as a sequence under a sort (or a root union over scans, filters and projections) and as a multiset otherwise, Float64 by
its bits, Timestamp as Int64, Utf8 as bytes.

The CPU tests hold the interpreter to what is already pinned (the reference's transcribed vectors, every *_ref module on its own table), every case
of the corpus to `explain` (no refusal) and to the interpreter (no NotImplementedError), and every quirk of plan_interp.QUIRKS to at least one case of
the stratum named next to it that tells it from the true rule."""
import functools
import json
import os
import struct

import numpy as np
import pyarrow as pa
import pytest

import plan_corpus as pc
import plan_interp as pi
from oracle import generic_ops as g
from plan_interp import run_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")
SEEDS = [0, 1, 2, 3]
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string()}


def _arrow(t):
    return pa.timestamp("ms") if isinstance(t, dict) else _PA[t]


@functools.lru_cache(maxsize=None)
def _case(stratum, seed, i):
    return pc.case(stratum, seed, i)


@functools.lru_cache(maxsize=None)
def _want(stratum, seed, i):
    """(names, types, rows) of the case, computed once and shared; an ExprError comes back as the exception object"""
    c = _case(stratum, seed, i)
    try:
        return run_plan(c.plan, c.tables)
    except g.ExprError as e:
        return e


def _norm(rows):
    """floats by their bits (-0.0 is not 0.0), text as bytes"""
    def one(v):
        if isinstance(v, float):
            return ("f", struct.unpack("<q", struct.pack("<d", v))[0])
        return v.encode() if isinstance(v, str) else v
    return [tuple(one(v) for v in r) for r in rows]


def _multiset(rows):
    return sorted(rows, key=lambda r: tuple((0, 0) if v is None else (1, repr(type(v)), v) for v in r))


def _plain(v):
    return v.item() if hasattr(v, "item") else v


# ------------------------------------------------------------------ CPU 1: the interpreter against what is already pinned
def test_interpreter_gives_the_transcribed_vectors_of_the_reference():
    import test_oracle_goldens as G
    t8 = {k: G.T8[k] for k in ("c1", "c2", "c3")}
    want = [(90, 92.1, "a"), (101, 96.4, "b"), (91, 95.3, "d")]                                 # context.rs:493-503
    names, types, rows = run_plan(json.load(open(os.path.join(PLANS, "golden_aggregate_sorted.json"))), [t8])
    assert (names, types, rows) == (["MAX(c1)", "MIN(c2)", "c3"], ["Int64", "Float64", "Utf8"], want)
    names, _, rows = run_plan(json.load(open(os.path.join(PLANS, "golden_aggregate.json"))), [t8])
    assert names == ["MAX(c1)", "MIN(c2)", "c3"] and sorted(rows, key=lambda r: r[2]) == want
    t1 = {"a": ["a", "b", "c", "d"], "b": [1, 10, 10, 100]}
    t2 = {"c": ["a", "b", "c", "d"], "d": [1, 10, 10, 100]}
    names, _, rows = run_plan(json.load(open(os.path.join(PLANS, "golden_join_sorted.json"))), [t1, t2])
    assert names == ["a", "b", "d"] and rows == [("a", 1, 1), ("b", 10, 10), ("c", 10, 10)]    # context.rs:579-589
    names, _, rows = run_plan(json.load(open(os.path.join(PLANS, "golden_join.json"))), [t1, t2])
    assert sorted(rows) == [("a", 1, 1), ("b", 10, 10), ("c", 10, 10), ("d", 100, 100)]
    _, _, rows = run_plan(json.load(open(os.path.join(PLANS, "sort_limit.json"))), [{"c1": G.T8["c1"]}])
    assert rows == [(90,), (90,), (91,)]
    # local.rs:223-231: SELECT MIN(c1), AVG(c4), COUNT(c3) -> 90 | 37.125 | 8 (no fixture holds this plan: the corpus' builder writes it)
    cols = [("c1", "Int64"), ("c3", "Utf8"), ("c4", "Int64")]
    node = pc.aggregate(pc.scan(cols), [], [("min", "c1"), ("avg", "c4"), ("count", "c3")])
    assert run_plan(node.plan, [{k: G.T8[k] for k in ("c1", "c3", "c4")}])[2] == [(90, 37.125, 8)]


def test_interpreter_equals_count_distinct_ref():
    import count_distinct_ref as ref
    import test_plan_count_distinct as D
    t = D.make_table(500, 3, null_p=0.3)
    for keys, aggs in (([], [("dc", "l"), ("count", None), ("dc", "s")]), (["kn", "ks"], [("dc", "i"), ("avg", "i"), ("dc", "u"), ("max", "t")])):
        names, _, rows = run_plan(D.whole_plan(keys, aggs), [t])
        assert names == keys + [ref.agg_name(f, a) for f, a in aggs]
        assert ref.sort_rows(rows, len(keys)) == ref.sort_rows(ref.aggregate(t, keys, aggs), len(keys))


def test_interpreter_equals_wide_group_ref():
    import test_plan_wide_group_by as W
    import wide_group_ref as ref
    t = W.make_table(700, 5, null_p=0.15)
    t = {k: [_plain(v) for v in vs] for k, vs in t.items()}
    for name in ("a9", "a16_sums"):
        _, _, rows = run_plan(W.whole_plan(["kn", "k2"], W.LISTS[name]), [t])
        assert ref.same_rows(ref.sort_rows(rows, 2), W.want_rows(t, ["kn", "k2"], W.LISTS[name]))


def test_interpreter_equals_global_agg_ref():
    import global_agg_ref as ref
    import test_plan_global_aggregates as A
    cols = A.make_table(200, 7, 0.2)
    aggs = [("count", None), ("count", "f"), ("sum", "i"), ("min", "u"), ("max", "t"), ("avg", "l"), ("min", "f")]
    t = ref.as_lists(cols)
    t["s"] = [""] * 200
    assert list(run_plan(A.whole_plan(aggs), [t])[2][0]) == ref.reference_row(cols, aggs)
    empty = {k: [] for k in t}
    assert list(run_plan(A.whole_plan(aggs), [empty])[2][0]) == [0, 0, None, None, None, None, None]


def test_interpreter_equals_semi_anti_ref_and_the_inner_join():
    import semi_anti_ref as ref
    import test_plan_composite_keys as K
    import test_plan_semi_anti as S
    left, right = S._table(300, 1, 40, null_p=0.1), {k + "_r": v for k, v in S._table(200, 2, 40, null_p=0.1).items()}
    for on in ([("l", "l_r")], [("i", "i_r"), ("s", "s_r")]):
        for jt in ("Semi", "Anti"):
            names, _, rows = run_plan(S._semi_plan(jt, on), [left, right])
            assert names == S.NAMES and rows == ref.table_rows(ref.semi_anti_table(left, right, on, jt == "Anti"), S.NAMES)
        _, _, rows = run_plan(K._join_plan(S.COLS, S.RCOLS, on), [left, right])
        assert sorted(rows, key=repr) == sorted(g.rows(g.hash_join_inner(left, right, on)), key=repr)


def test_interpreter_equals_cross_join_ref():
    import cross_join_ref as ref
    import test_plan_cross_join as X
    left, right = X.make_table(9, 1, 0.2), X.make_table(4, 2, 0.2, suffix="_r")
    names, _, rows = run_plan(X._cross(X._scan(X.COLS), X._scan(X.RCOLS), X.COLS, X.RCOLS), [left, right])
    assert names == X.NAMES + X.RNAMES and X._norm(rows) == X._norm(ref.cross_rows(ref.rows_of(left, X.NAMES), ref.rows_of(right, X.RNAMES)))


def test_interpreter_equals_scalar_fn_text_expr_and_text_slice_ref():
    import scalar_fn_ref as sref
    import test_plan_text_expr as T
    import test_plan_text_slices as L
    import text_expr_ref as tref
    import text_slice_ref as lref
    t = T.make_table(400, 9)
    t["t"] = [None if v is None else v - 1_450_000_000_000 for v in t["t"]]              # (either side of 1970)
    fns = [sref.fn(m, T.c("f")) for m in sref.MATH if m != "sqrt"] + [sref.fn("date_trunc", sref.lit_utf8(u), T.c("t")) for u in sref.TRUNC_UNITS]
    fns += [sref.fn("date_part", sref.lit_utf8(u), T.c("t")) for u in sref.PART_UNITS] + [sref.fn("char_length", T.c("s")), sref.fn("octet_length", T.c("s"))]
    fns.append(T.binary(sref.fn("floor", T.c("f")), "Plus", T.cast(sref.fn("date_part", sref.lit_utf8("dow"), T.c("t")), "Float64")))
    plan = T.projection([(e, "x%d" % k) for k, e in enumerate(fns)], out_types={"x%d" % k: sref.result_type("abs") for k in range(len(fns))})
    _, _, rows = run_plan(plan, [t])
    for k, e in enumerate(fns):
        assert [sref.bits(r[k]) for r in rows] == [sref.bits(v) for v in sref.eval_rows(e, t, T.TYPES)], k
    _, _, rows = run_plan(T.projection([(T.mixed_case(), "x")]), [t])
    assert [r[0] for r in rows] == tref.eval_text(T.mixed_case(), t, T.TYPES)
    lt = L.make_table(400, 4)
    _, types, rows = run_plan(L.projection([(e, "x%d" % k) for k, e in enumerate(L.EVERY)]), [lt])
    assert set(types) == {"Utf8"}
    for k, e in enumerate(L.EVERY):
        assert [r[k] for r in rows] == lref.eval_text(e, lt, L.TYPES), k


def test_interpreter_equals_the_like_reference_and_the_window_reference():
    import test_plan_like as K
    import test_plan_window_aggregates as W
    r = np.random.default_rng(5)
    vals = [None if k % 9 == 0 else "".join(r.choice(K.ALPHABET, r.integers(0, 7))) for k in range(600)]
    t = {"s": vals, "t": vals[::-1], "i": [k % 7 for k in range(600)], "k": list(range(600))}
    for pred in (K.like("s", "a%"), K.like("s", "%b_", True), K.binop("Or", K.like("t", "_é%"), K.binop("Lt", K.col("s"), K.lit("b"))),
                 K.binop("And", K.binop("GtEq", K.lit("bé"), K.col("t")), K.not_(K.like("s", "%c%")))):
        _, _, rows = run_plan(K.filter_plan(pred), [t])
        bt = {"s": [None if v is None else v.encode() for v in t["s"]], "t": [None if v is None else v.encode() for v in t["t"]], "i": t["i"], "k": t["k"]}
        assert [row[3] for row in rows] == K.expected_rows(pred, bt)
    n = 3000
    cols = W._sorted_table(n, 3, [5, 700, 1, 2049], 40, 0.2)
    t = {c: [v.item() if ok else None for v, ok in zip(*cols[c])] for c, _ in W.COLS if c != "s"}
    t["s"] = [""] * n
    entries = W._entries(["p"], ["o"]) + W._entries(["p"], []) + [W.row_number_entry(["p"])]
    names, _, rows = run_plan(W.window_plan(entries), [t])
    assert names[len(entries):] == [c for c, _ in W.COLS]
    for k, e in enumerate(entries[:-1]):
        a = e["aggregate"]
        want, ok = W.reference_window(cols, n, a["aggregate_expr"], a["expr"].get("name"), ["p"], ["o"] if e["order_by"] else [])
        assert [row[k] for row in rows] == [v.item() if o else None for v, o in zip(want, ok)], a["name"]
    p = t["p"]
    assert [row[len(entries) - 1] for row in rows] == [1 + i - max(j for j in range(i + 1) if j == 0 or p[j] != p[j - 1]) for i in range(n)]


def test_interpreter_equals_union_ref():
    import test_plan_union as U
    import union_ref as ref
    shape = (5, 0, 7, 3, 4)                                                                      # an empty input; NULLs in the odd inputs
    tabs = U._tables(shape, 3, True)
    scans = [U._scan(U._sfx(U.COLS, k)) for k in range(len(shape))]
    want = ref.union_rows([ref.rows_of(t, [c for c, _ in U._sfx(U.COLS, k)]) for k, t in enumerate(tabs)])
    assert any(v is None for r in want for v in r) and len(want) == sum(shape)
    for plan in (U._union(scans), U._union([scans[0], U._union([scans[1], U._union(scans[2:4])]), scans[4]])):      # flat, and unions under unions
        names, types, rows = run_plan(plan, tabs)
        assert names == U.NAMES and types == [U._dt(t) for _, t in U.COLS] and _norm(rows) == _norm(want)
    # one relation under two branches is ONE table (A-U7); a filter keeps its input's order
    bid = U._bids(3000, 20)
    names, _, rows = run_plan(json.load(open(os.path.join(PLANS, "bids_two_ranges.json"))), [bid])
    high = [a for a, p in zip(bid["auction"], bid["price"]) if p > 9_000_000]
    late = [b for b, t in zip(bid["bidder"], bid["b_date_time"]) if t > 1_436_918_400_000 + 50_000]
    assert names == ["id"] and [r[0] for r in rows] == ref.union_table([{"id": high}, {"bidder": late}])["id"] and high and not late
    for quirk in ("union_inputs_reversed", "union_is_distinct"):
        assert run_plan(U._union([scans[0], scans[0], scans[3]]), [tabs[0], tabs[3]], frozenset([quirk]))[2] != run_plan(U._union([scans[0], scans[0], scans[3]]), [tabs[0], tabs[3]])[2]


def test_interpreter_equals_cast_text_ref():
    import cast_text_ref as ref
    import test_plan_cast_text as K
    t = K.shared_table(300)
    q10 = [K.left(ref.cast_utf8(K.c("t")), 10), K.right(K.left(ref.cast_utf8(K.c("t")), 16), 5)]
    label = K.case([(K.mod("k", 3, 0), ref.cast_utf8(K.c("l"))), (K.mod("k", 3, 1), K.c("s"))], K.lit_utf8("none"))
    exprs = [ref.cast_utf8(K.c(n)) for n in "ilut"] + [ref.cast_utf8(K.c("w"), try_cast=True), ref.cast_utf8(K.binary(K.c("i"), "Multiply", K.lit("Int32", 2)))] + q10 + [label]
    _, types, rows = run_plan(K.projection([(e, "x%d" % k) for k, e in enumerate(exprs)]), [t])
    assert set(types) == {"Utf8"}
    for k, e in enumerate(exprs):
        assert [r[k] for r in rows] == ref.eval_text(e, t, K.TYPES), k
    assert any(r[4] is None and w is not None for r, w in zip(rows, t["w"]))                      # try_cast_expr beyond the years: NULL
    beyond = K.projection([(ref.cast_utf8(K.c("w")), "x")])                                      # cast_expr of the same column fails the call
    with pytest.raises(ref.CastRangeError):
        ref.eval_text(ref.cast_utf8(K.c("w")), t, K.TYPES)
    with pytest.raises(g.ExprError):
        run_plan(beyond, [t])


def test_interpreter_equals_parse_text_ref():
    import parse_text_ref as ref
    import test_plan_parse_text as P
    vals = ref.corpus()
    t = {"k": list(range(len(vals))), "s": [None if k % 50 == 7 else v for k, v in enumerate(vals)], "d": [None] * len(vals), "i": [0] * len(vals)}
    targets = [(ty, ref.TS if ty == "Timestamp" else ty) for ty in ref.TARGETS]
    plan = P.projection([(ref.cast_to(P.c("s"), ty, try_cast=True), "x" + ty, full) for ty, full in targets])
    _, types, rows = run_plan(plan, [t])
    assert types == [full for _, full in targets]
    for k, (ty, _) in enumerate(targets):
        want = ref.parse(t["s"], ty, try_cast=True)
        assert [r[k] for r in rows] == want and 100 < sum(v is not None for v in want) < len(vals) - 100, ty
        with pytest.raises(ref.ParseError):
            ref.parse(t["s"], ty)
        with pytest.raises(g.ExprError):                                                         # cast_expr: one value that does not parse fails the call
            run_plan(P.projection([(ref.cast_to(P.c("s"), ty), "x", targets[k][1])]), [t])
        good = dict(t, s=[v if w is not None else None for v, w in zip(t["s"], want)])
        assert [r[0] for r in run_plan(P.projection([(ref.cast_to(P.c("s"), ty), "x", targets[k][1])]), [good])[2]] == ref.parse(good["s"], ty) == want


def _relation(fields, n, **cols):
    """a table for a fixture's leaf: the named columns, every other field NULL"""
    return {f["name"]: list(cols.get(f["name"], [None] * n)) for f in fields}


def test_interpreter_gives_what_the_three_fixtures_tests_expect():
    import cast_text_ref as cref
    import test_plan_union as U
    r = np.random.default_rng(5)
    # person_activity.json as tests/test_plan_union.py expects it: a count per (person, kind)
    plan = json.load(open(os.path.join(PLANS, "person_activity.json")))
    fa, fb = pi.leaf_schemas(plan)
    na, nb = 700, 1300
    seller = [int(x) for x in r.integers(0, 40, na)]
    bid = U._bids(nb, 6)
    bid["bidder"] = [b % 60 for b in bid["bidder"]]
    names, _, rows = run_plan(plan, [_relation(fa, na, a_date_time=[1_436_918_400_000 + 11 * k for k in range(na)], seller=seller), _relation(fb, nb, **bid)])
    want = {}
    for p, kind in [(s, "auction") for s in seller] + [(b, "bid") for b in bid["bidder"]]:
        want[(p, kind)] = want.get((p, kind), 0) + 1
    assert names == ["person", "kind", "COUNT(UInt8(1))"] and sorted(rows) == sorted((p, k, n) for (p, k), n in want.items()) and len(want) == 100
    # q10_date_time_text.json as tests/test_plan_cast_text.py expects it: the date and the time of day out of the timestamp's text
    plan = json.load(open(os.path.join(PLANS, "q10_date_time_text.json")))
    n = 2000
    ms = [1_699_920_000_000 + int(d) * 86_400_000 + int(x) for d, x in zip(r.integers(0, 3, n), r.integers(-2000, 2001, n))]      # within two seconds of a midnight
    bid = {"auction": list(range(n)), "bidder": [j % 13 for j in range(n)], "price": [(j * 37) % 10_000 for j in range(n)], "b_date_time": ms}
    names, _, rows = run_plan(plan, [bid])
    text = cref.ts_text(ms)
    assert names == ["auction", "bidder", "price", "b_date_time", "date", "time"]
    assert rows == [(bid["auction"][j], bid["bidder"][j], bid["price"][j], ms[j], text[j][:10], text[j][11:16]) for j in range(n)]
    assert {"23:59", "00:00"} <= {row[5] for row in rows} and {len(s) for s in text} == {19, 23}
    # person_card_prefix.json as tests/test_plan_parse_text.py expects it: a count per four-digit prefix
    plan = json.load(open(os.path.join(PLANS, "person_card_prefix.json")))
    n = 3000
    cards = ["%04d %04d %04d %04d" % ((j * j) % 50 * 199, j % 10_000, 0, j % 3) for j in range(n)]
    names, types, rows = run_plan(plan, [_relation(pi.leaf_schemas(plan)[0], n, credit_card=cards)])
    want = {}
    for s in cards:
        want[int(s[:4])] = want.get(int(s[:4]), 0) + 1
    assert names == ["prefix", "COUNT(UInt8(1))"] and types[0] == "Int32" and sorted(rows) == sorted(want.items()) and len(want) > 20


# ------------------------------------------------------------------ CPU 2: every case explains and evaluates
def _leaf(node):
    while node["execution_plan"] != "memory_exec":
        node = node["input"]
    return node


def test_the_corpus_has_its_floors():
    assert len(pc.STRATA) >= 19 and len(SEEDS) >= 4 and pc.CASES_PER_SEED >= 6 and set(pc.MUST_RUN) == set(pc.STRATA) == set(pc._RECIPES)
    assert set(pi.QUIRKS.values()) <= set(pc.STRATA)
    for s in pc.STRATA:
        sizes = [max(len(next(iter(t.values()))) for t in _case(s, seed, i).tables) for seed in SEEDS for i in range(pc.CASES_PER_SEED)]
        assert sizes.count(20_011) == 1 and sizes.count(32_769) == 1 and max(sizes) == 32_769, (s, sizes)
    # the edges the recipes promise: four PARTITION BY and four ORDER BY columns in every seed; an empty right side under Semi and under Anti; a join
    # build key on every row and on half of them; a leaf with a projection of its own; a filter over an aggregate; a union of more than 16 inputs, of
    # one relation twice, of an input without validity beside one with it; a parse through a slice and through a materialised text
    empty = set()
    for seed in SEEDS:
        w = _case("window", seed, 3).plan
        while w["execution_plan"] != "window_agg_exec":
            w = w["input"]
        assert any(len(e["partition_by"]) == 4 and len(e["order_by"]) == 4 for e in w["window_expr"]), seed
        c = _case("join_semi_anti", seed, 2)
        if not c.tables[1]["b_id"]:
            empty.add("Semi" if '"join_type": "Semi"' in json.dumps(c.plan) else "Anti")
        assert any(len(f["projection"]) < len(f["schema"]["fields"]) for i in range(pc.CASES_PER_SEED)
                   for f in [_leaf(_case("sort_limit", seed, i).plan)]), seed
        assert _case("group_narrow", seed, 3).plan["input"]["execution_plan"] == "filter_exec"
        assert any(len(u["inputs"]) > 16 for u in _nodes(_case("union", seed, 3).plan, "union_exec")), seed
        c = _case("union", seed, 1)
        assert c.plan["execution_plan"] == "union_exec" and len(c.tables) == 1 and len(pi.leaf_schemas(c.plan)) == 1, seed
        assert len(_nodes(c.plan, "memory_exec")) == 2 and c.ordered
        c = _case("union", seed, 0)
        plain = [all(v is not None for col in t.values() for v in col) for t in c.tables]
        assert c.plan["execution_plan"] == "union_exec" and sorted(plain) == [False, True] and c.ordered, (seed, plain)
        assert {len(next(iter(t.values()))) for t in c.tables} <= set(pc.UNION_ROWS)
        roles = [[_text_kind(e["expr"]) for e in _exprs(_case("parse_text", seed, i).plan) if _parses_text(e)] for i in (2, 3)]
        assert "slice" in roles[0] and "materialised" in roles[1], (seed, roles)
    assert empty == {"Semi", "Anti"}
    # every directed value of the casts to text, and every entry of parse_text_ref's edge table, stands non-NULL in some seed
    for c, pool in pc.number_pools().items():
        assert set(pool) <= {v for seed in SEEDS for v in _case("cast_text", seed, 0).tables[0]["a_" + c]}, c
    assert {len(str(v).lstrip("-")) for v in pc.number_pools()["u"]} == set(range(1, 21))
    import parse_text_ref as ptref
    for name in ("a_n", "a_d"):
        assert set(ptref.EDGES) <= {v for seed in SEEDS for v in _case("parse_text", seed, 1).tables[0][name]}, name
    notes = " ".join(_case(s, seed, 2).note for s in ("join_inner", "join_semi_anti") for seed in SEEDS)
    assert "(hot)" in notes and "(constant)" in notes and "(repeat)" in notes


def _nodes(plan, kind):
    """every node of `kind` in the plan, depth first"""
    out = [plan] if plan.get("execution_plan") == kind else []
    for k in ("input", "left", "right"):
        if isinstance(plan.get(k), dict):
            out += _nodes(plan[k], kind)
    for x in plan.get("inputs") or ():
        out += _nodes(x, kind)
    return out


def _exprs(x):
    """every expression object anywhere in a plan"""
    if isinstance(x, dict):
        if "physical_expr" in x:
            yield x
        for v in x.values():
            yield from _exprs(v)
    elif isinstance(x, list):
        for v in x:
            yield from _exprs(v)


def _parses_text(e):
    return e["physical_expr"] in ("cast_expr", "try_cast_expr") and e["cast_type"] != "Utf8" and _text_kind(e["expr"]) is not None


def _text_kind(e):
    """'column' | 'slice' (a chain of slice functions over a column: read in place) | 'materialised' (a text CASE, a number cast to Utf8, a slice of
    those) | None for what is no text"""
    t = e["physical_expr"]
    if t == "column":
        return "column" if e["name"] in dict(pc.PARSE_COLS) or e["name"].endswith(("_s", "_s2")) else None
    if t == "scalar_function_expr" and e["name"] in pi.tsl.SLICE_FNS:
        below = _text_kind(e["args"][0])
        return "slice" if below in ("column", "slice") else below
    if t == "case_expr":
        return "materialised" if any(_text_kind(th) for _, th in e["when_then_expr"]) else None
    if t in ("cast_expr", "try_cast_expr") and e["cast_type"] == "Utf8":
        return "materialised"
    return None


@pytest.mark.parametrize("stratum", pc.STRATA)
def test_every_case_explains_and_evaluates(stratum):
    """zero refusals from flockgpu_plan_explain, no NotImplementedError from the interpreter; a case of an error stratum raises ExprError and nothing
    else does; `ordered` exactly where the root fixes the row order (a sort, a limit over one, a union over scans, filters and projections); the
    schema explain derives for the root is the interpreter's"""
    from flock_amd.runtime import explain
    for seed in SEEDS:
        for i in range(pc.CASES_PER_SEED):
            c = _case(stratum, seed, i)
            text = explain(c.plan)                                # raises FlockGpuError on a refusal
            want = _want(stratum, seed, i)
            assert isinstance(want, g.ExprError) == (stratum in pc.ERROR_STRATA), (stratum, seed, i, c.note, want if isinstance(want, Exception) else "")
            assert c.ordered == (c.plan["execution_plan"] == "sort_exec" or (c.plan["execution_plan"] == "global_limit_exec" and c.plan["input"]["execution_plan"] == "sort_exec")
                                 or pc.ordered_union(c.plan))
            for cut, t in zip(c.batch_cuts, c.tables):
                n = len(next(iter(t.values())))
                assert cut[0] == 0 and cut[-1] == n and cut == sorted(cut) and any(a == b for a, b in zip(cut, cut[1:])), (stratum, seed, i, cut)
            if isinstance(want, Exception):
                continue
            names, types, rows = want
            assert len(rows) <= 120_000, (stratum, seed, i, len(rows))
            head = text.split("\n")[0]
            shown = head[head.index("[") + 1:head.rindex("]")] if "[" in head else None
            mine = ", ".join("%s:%s" % (n, "Timestamp(ms)" if isinstance(t, dict) else t) for n, t in zip(names, types))
            assert shown == mine, (stratum, seed, i, c.note, head, mine)


# ------------------------------------------------------------------ CPU 3: the corpus tells neighbours apart
@pytest.mark.parametrize("quirk", sorted(pi.QUIRKS))
def test_some_case_of_its_stratum_detects_the_quirk(quirk):
    stratum = pi.QUIRKS[quirk]
    for seed in SEEDS:
        for i in range(pc.CASES_PER_SEED):
            c = _case(stratum, seed, i)
            if len(next(iter(c.tables[0].values()))) > 9000:
                continue                                          # (the small cases are enough, and quicker)
            names, types, rows = _want(stratum, seed, i)
            try:
                qn, qt, qrows = run_plan(c.plan, c.tables, frozenset([quirk]))
            except g.ExprError:
                return                                            # the wrong rule fails a call that the true rule completes

            a, b = _norm(rows), _norm(qrows)
            if (a != b) if c.ordered else (_multiset(a) != _multiset(b)):
                return
    pytest.fail("no case of stratum %s tells quirk %s from the true rule" % (stratum, quirk))


def test_an_unknown_quirk_and_a_node_outside_the_dialect_are_named():
    with pytest.raises(ValueError, match="no_such_quirk"):
        run_plan(_case("cross", 0, 1).plan, _case("cross", 0, 1).tables, frozenset(["no_such_quirk"]))
    with pytest.raises(NotImplementedError, match="sort_preserving_merge_exec"):
        run_plan({"execution_plan": "sort_preserving_merge_exec", "input": _case("cross", 0, 1).plan}, _case("cross", 0, 1).tables)
    a = pc.scan([("x", "Int32")])
    with pytest.raises(NotImplementedError, match="Left"):
        run_plan(dict(pc.join("Inner", a, pc.scan([("y", "Int32")]), [("x", "y")]).plan, join_type="Left"), [{"x": [1]}, {"y": [1]}])
    with pytest.raises(NotImplementedError, match="lower"):
        run_plan(pc.proj(pc.scan([("s", "Utf8")]), [(pc.fn("lower", "Utf8", pc.col("s", [("s", "Utf8")])), "x", "Utf8")]).plan, [{"s": ["A"]}])


# ------------------------------------------------------------------ CPU 4: case is a pure function
def test_case_is_a_pure_function_of_its_arguments():
    for stratum in pc.STRATA:
        for seed, i in ((0, 0), (1, 4), (3, 5)):
            a, b = pc.case(stratum, seed, i), pc.case(stratum, seed, i)
            assert json.dumps(a.plan, sort_keys=True) == json.dumps(b.plan, sort_keys=True) and a.batch_cuts == b.batch_cuts
            assert _norm_tables(a.tables) == _norm_tables(b.tables) and (a.ordered, a.note) == (b.ordered, b.note)
        assert json.dumps(pc.case(stratum, 0, 0).plan) != json.dumps(pc.case(stratum, 1, 0).plan) or pc.case(stratum, 0, 0).tables != pc.case(stratum, 1, 0).tables


def _norm_tables(tables):
    return [{k: _norm([tuple(v)])[0] for k, v in t.items()} for t in tables]


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


def _batches(plan, tables, cuts_per_table):
    """per leaf (in the interpreter's leaf order) the list of record batches: one batch, or one per pair of neighbouring cuts"""
    out = []
    for fields, t, cuts in zip(pi.leaf_schemas(plan), tables, cuts_per_table):
        n = len(t[fields[0]["name"]])
        cuts = cuts or [0, n]
        bs = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            arrs = []
            for f in fields:
                ty = _arrow(f["data_type"])
                arrs.append(pa.array(t[f["name"]][a:b], pa.int64()).cast(ty) if pa.types.is_timestamp(ty) else pa.array(t[f["name"]][a:b], ty))
            bs.append(pa.record_batch(arrs, names=[f["name"] for f in fields]))
        out.append(bs)
    return out


def _execute(gpu, plan, feeds, generic_only):
    """-> (schema or None when no batch came back, rows, the names of the kernels that ran)"""
    from flock_amd.runtime import ExecutionContext, collect
    ctx = ExecutionContext([plan], gpu=gpu, generic_only=generic_only)
    gpu.profile_reset()
    gpu.profile(True)
    try:
        out = collect(ctx, [[f] for f in feeds])[0]
        ran = set(gpu.profile_read())
    finally:
        gpu.profile(False)
        ctx.close()
    rows = []
    for rb in out:
        cols = [(c.cast(pa.int64()) if pa.types.is_timestamp(c.type) else c).to_pylist() for c in rb.columns]
        rows += list(zip(*cols)) if cols else []
    return (out[0].schema if len(out) else None), rows, ran


def _compare(gpu, key, ran_all):
    """one case, whole and in batches, against the interpreter: the failure message carries everything needed to reproduce it without a GPU"""
    from flock_amd.runtime import explain
    stratum, seed, i = key
    c = _case(*key)
    names, types, rows = _want(*key)
    want = _norm(rows)
    if not c.ordered:
        want = _multiset(want)
    for how, cuts in (("whole", [None] * len(c.tables)), ("batches", c.batch_cuts)):
        schema, got, ran = _execute(gpu, c.plan, _batches(c.plan, c.tables, cuts), pc.generic_only(*key))
        ran_all |= ran
        where = "case%r %s (%s), generic_only=%s\n%s" % (key, how, c.note, pc.generic_only(*key), explain(c.plan))
        if schema is not None:
            assert schema.names == names, where
            assert [f.type for f in schema] == [_arrow(t) for t in types], where
        else:
            assert not rows, where
        got = _norm(got)
        if not c.ordered:
            got = _multiset(got)
        if got != want:
            diff = [(k, a, b) for k, (a, b) in enumerate(zip(got, want)) if a != b][:3]
            pytest.fail("%d rows, %d expected; first differing (position, got, expected): %r\n%s" % (len(got), len(want), diff or (got[len(want):][:3], want[len(got):][:3]), where))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("stratum", [s for s in pc.STRATA if s not in pc.ERROR_STRATA])
def test_gpu_equals_the_interpreter(gpu, stratum, seed):
    ran = set()
    for i in range(pc.CASES_PER_SEED):
        _compare(gpu, (stratum, seed, i), ran)
    print("\n%s seed %d ran: %s" % (stratum, seed, " ".join(sorted(ran))))
    missing = [k for k in pc.MUST_RUN[stratum] if not any(name.startswith(k) for name in ran)]      # by prefix: sort_emit_kernel is one template, many names
    assert not missing, (stratum, seed, missing, sorted(ran))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("stratum", pc.ERROR_STRATA)
def test_gpu_fails_the_call_on_the_one_bad_row_and_is_correct_afterwards(gpu, stratum, seed):
    from flock_amd import FlockGpuError, _ffi
    ran = set()
    for i in range(pc.CASES_PER_SEED):
        key = (stratum, seed, i)
        c = _case(*key)
        assert isinstance(_want(*key), g.ExprError)
        for cuts in ([None], c.batch_cuts):
            with pytest.raises(FlockGpuError) as e:
                _execute(gpu, c.plan, _batches(c.plan, c.tables, cuts), pc.generic_only(*key))
            assert e.value.code == _ffi.ERR_INVALID, (key, c.note, str(e.value))
        _compare(gpu, ("filter_project", seed, 3), ran)          # the next case on the same GpuContext is correct


# ------------------------------------------------------------------ findings, reduced: literal plans and tables, no generator
@pytest.mark.gpu
def test_like_beside_a_computed_leaf_is_refused_by_name(gpu):
    """Found by filter_project (seed 0, case 0): `s LIKE '%w%' AND (i % 2) IS NOT NULL`.  IS NOT NULL of a computed value is no leaf of the one-pass
    predicate program, so the whole predicate goes to the general evaluator, which takes no text: the execute is refused with
    FLOCKGPU_ERR_UNSUPPORTED naming the operator (the README's text-predicate limits).  What must never happen is a wrong answer: the interpreter's
    is [(1,)].  The same LIKE beside `i % 2 = 1`, a leaf of the program, executes."""
    from flock_amd import FlockGpuError, _ffi
    cols = [("s", "Utf8"), ("i", "Int32"), ("k", "Int64")]
    t = {"s": ["w", "aw", None, "x"], "i": [2, None, 3, 5], "k": [1, 2, 3, 4]}
    a = pc.scan(cols)
    like = pc.binop(a.c("s"), "Like", pc.lit("Utf8", "%w%"))
    rem = pc.binop(a.c("i"), "Modulo", pc.lit("Int32", 2))
    computed = pc.keep(pc.filt(a, pc.binop(like, "And", {"physical_expr": "is_not_null_expr", "arg": rem})), ["k"])
    assert run_plan(computed.plan, [t])[2] == [(1,)]
    with pytest.raises(FlockGpuError) as e:
        _execute(gpu, computed.plan, _batches(computed.plan, [t], [None]), True)
    assert e.value.code == _ffi.ERR_UNSUPPORTED and "Like" in str(e.value), str(e.value)
    leaf = pc.keep(pc.filt(a, pc.binop(like, "And", pc.binop(rem, "Eq", pc.lit("Int32", 0)))), ["k"])
    _, rows, _ = _execute(gpu, leaf.plan, _batches(leaf.plan, [t], [None]), True)
    assert rows == run_plan(leaf.plan, [t])[2] == [(1,)]
