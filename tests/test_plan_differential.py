"""Random plans over the generic operators against a CPU interpreter: tests/plan_corpus.py draws plans inside the claimed dialect, tests/plan_interp.py
evaluates them row at a time, the GPU tests run them through ExecutionContext + collect -- whole and cut into batches -- and compare EXACTLY: schema
names and Arrow types, rows as a sequence under a sort (or a root union over scans, filters and projections) and as a multiset otherwise, Float64 by
its bits, Timestamp as Int64, Utf8 as bytes.

The CPU tests hold the interpreter to what is already pinned (the reference's transcribed vectors, every *_ref module on its own table), every case
of the corpus to `explain` (no refusal) and to the interpreter (no NotImplementedError), and every quirk of plan_interp.QUIRKS to at least one case of
the stratum named next to it that tells it from the true rule.

What lies under a NULL is tests/null_poison.py's: the same cases run once more with near and far values in every NULL slot of every fed column
(validity alone decides), after the CPU tests have shown that those values, read, would change the answer; literal plans put what FAILS a live row
under NULLs."""
import functools
import json
import os
import struct

import numpy as np
import pyarrow as pa
import pytest

import null_poison as npz
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


# ------------------------------------------------------------------ CPU 2b: what lies under a NULL (tests/null_poison.py)
NULL_STRATA = [s for s in pc.STRATA if s not in pc.ERROR_STRATA]
POISON_TYPES = ("Int32", "Int64", "UInt64", "Timestamp", "Float64", "Utf8")


def _keys_of(stratum):
    return [(stratum, seed, i) for seed in SEEDS for i in range(pc.CASES_PER_SEED)]


def _rows_of_case(key):
    return max(len(next(iter(t.values()))) for t in _case(*key).tables)


def _unmasked_tables(key, pool, only=None):
    """the case's tables with every NULL (of the columns of type `only`, or of every column) replaced by its poison AS A LIVE VALUE; None where that
    changes nothing (no such NULL)"""
    c = _case(*key)
    out, changed = [], False
    for leaf, (fields, t) in enumerate(zip(pi.leaf_schemas(c.plan), c.tables)):
        u = dict(t)
        for f in fields:
            if (only is None or npz.type_name(f["data_type"]) == only) and any(v is None for v in t[f["name"]]):
                u[f["name"]] = npz.unmasked(pool, key, leaf, f["name"], t[f["name"]], f["data_type"])
                changed = True
        out.append(u)
    return out if changed else None


@functools.lru_cache(maxsize=None)
def _detects(key, pool, only=None):
    """would the interpreter's answer change (or the run fail) if the poison of this pool were read as values?"""
    c = _case(*key)
    tables = _unmasked_tables(key, pool, only)
    if tables is None:
        return False
    try:
        rows = run_plan(c.plan, tables)[2]
    except Exception:                                             # ExprError from a divisor or a cast, OverflowError from a date beyond datetime, ...
        return True
    a, b = _norm(rows), _norm(_want(*key)[2])
    return (a != b) if c.ordered else (_multiset(a) != _multiset(b))


def test_the_far_pool_holds_what_it_promises():
    from test_plan_like import reference_like
    import parse_text_ref as ptref
    far = npz.FAR
    for pattern in pc.LIKES:
        assert pattern == "" or any(reference_like(s, pattern) for s in far["Utf8"]), pattern
    assert {len(s) for s in far["Utf8"]} >= {17, 70} and {b"12x", b"99999999999999999999", b"a/b/c", b"\xff\xfe", b"\x80", b"\xe2\x82"} <= set(far["Utf8"])
    for s in (b"\xff\xfe", b"\x80", b"\xe2\x82"):
        with pytest.raises(UnicodeDecodeError):
            s.decode()
    assert all(ptref.parse_one(s, t) is None for s in ("12x", "99999999999999999999") for t in ptref.TARGETS)
    assert {-2**31, 2**31 - 1, -1, 0x55555555, 0} <= set(far["Int32"]) and {-2**63, 2**63 - 1, -1, 0x5555555555555555, 2**40, 0} <= set(far["Int64"])
    assert {0, 2**64 - 1, 0x5555555555555555, 2**40} <= set(far["UInt64"])
    assert {pc.TS_MAX + 1, pc.TS_MIN - 1, -2**63, 2**63 - 1, 0} <= set(far["Timestamp"])
    bits = {struct.unpack("<Q", struct.pack("<d", v))[0] for v in far["Float64"]}
    assert bits >= {0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000, 1, 0x7FEFFFFFFFFFFFFF, 0}


@pytest.mark.parametrize("stratum", pc.STRATA)
def test_poisoned_batches_read_as_the_plain_ones_and_differ_in_their_buffers(stratum):
    """for every case and both pools: every poisoned column equals the plain one as Arrow compares (and by to_pylist() in the cases of at most 9000
    rows), null_count is the number of Nones, the array validates in full -- bytes that are no UTF-8 under a NULL included --, and its buffers DIFFER
    from pyarrow's: asserted for every column with at least 8 NULLs under far (a draw of 0 is one of five at the most) and with at least 32 NULLs
    and a live value other than 0 / '' under near (a near pool is the live values and 0).  No near poison moves the minimum or maximum over all
    slots; slot() agrees with slots(); the slots do not depend on how the table is cut"""
    for key in _keys_of(stratum):
        c = _case(*key)
        small = _rows_of_case(key) <= 9000
        plain = _batches(c.plan, c.tables, [None] * len(c.tables))
        for pool in npz.POOLS:
            got = _batches(c.plan, c.tables, [None] * len(c.tables), poison=(pool, key))
            for leaf, (fields, t) in enumerate(zip(pi.leaf_schemas(c.plan), c.tables)):
                a, b = plain[leaf][0], got[leaf][0]
                assert a.schema == b.schema
                for f, x, y in zip(fields, a.columns, b.columns):
                    where = (key, pool, f["name"])
                    vals = t[f["name"]]
                    ty = npz.type_name(f["data_type"])
                    y.validate(full=True)
                    assert y.null_count == x.null_count == sum(v is None for v in vals), where
                    if ty == "Float64" or small:                  # (Arrow's equals takes a live NaN for unequal to itself; datetime ends before the far timestamps)
                        x64, y64 = (x.cast(pa.int64()), y.cast(pa.int64())) if ty == "Timestamp" else (x, y)
                        a_list, b_list = y64.to_pylist(), x64.to_pylist()
                        assert (_norm([tuple(a_list)]) == _norm([tuple(b_list)])) if ty == "Float64" else (a_list == b_list), where
                    if ty != "Float64":
                        assert y.equals(x), where
                    if not y.null_count:
                        continue
                    live = [v for v in vals if v is not None and v == v]
                    if y.null_count >= (8 if pool == "far" else 32) and (pool == "far" or any(v not in (0, "") for v in live)):
                        assert [bytes(m) for m in y.buffers()[1:]] != [bytes(m) for m in x.buffers()[1:]], where
                    if not small:
                        continue
                    under = npz.slots(pool, *key, leaf, f["name"], vals, ty)
                    if pool == "near" and ty != "Utf8" and live:
                        s = [v for v in under if v == v]
                        assert min(s) == min(live) and max(s) == max(live), where
                    k = vals.index(None)
                    assert _norm([(npz.slot(pool, *key, leaf, f["name"], k, vals, ty),)]) == _norm([(under[k],)]), where
        if not small:
            continue
        cut = _batches(c.plan, c.tables, c.batch_cuts, poison=("far", key))
        whole = _batches(c.plan, c.tables, [None] * len(c.tables), poison=("far", key))
        for bs, w in zip(cut, whole):
            for j, col in enumerate(w[0].columns):
                parts = [b.column(j) for b in bs]
                at = 2 if pa.types.is_string(col.type) else 1
                assert pa.concat_arrays(parts).null_count == col.null_count, key
                assert b"".join(p.buffers()[at].to_pybytes() for p in parts) == col.buffers()[at].to_pybytes(), key


SENSITIVITY_PER_SEED, SENSITIVITY_PER_STRATUM = 2, 12


@pytest.mark.parametrize("stratum", NULL_STRATA)
def test_the_poison_would_change_the_answer_if_it_were_read(stratum):
    """Sensitivity: what makes test_gpu_ignores_what_lies_under_a_null mean something.  Every None of a case's tables is replaced by its poison AS A
    LIVE VALUE and the interpreter runs the case: it must give another result than _want, or raise.  Such a case `detects` (under either pool: the
    GPU test feeds both).  Asserted: every (stratum, seed) has at least 2 detecting cases of 6, every stratum at least 12 of 24.

    The cases are tried smallest first and the count stops where both floors are met, which keeps the two cases of 20 011 and 32 769 rows out of
    most strata; all four seeds are checked.  The full counts, from a run without that stop (cases of 24 detecting under near, under far, under
    either; then the cases of 6 per seed 0 .. 3 under either):

    stratum          near far either  per seed (either)
    filter_project     17  19     19  4 6 4 5
    text               17  16     17  4 4 5 4
    group_narrow       18  18     18  5 5 5 3
    group_composite    20  21     21  5 6 6 4
    group_wide         23  23     23  6 6 5 6
    distinct_count     19  21     21  5 6 5 5
    global_agg         11  16     16  4 4 6 2
    join_inner         23  22     23  6 6 5 6
    join_semi_anti     23  21     23  6 6 6 5
    sort_limit         22  22     22  5 5 6 6
    window             22  22     22  6 6 5 5
    cross              16  19     19  5 5 5 4
    mixed              21  21     22  6 5 6 5
    union              23  23     23  6 6 6 5
    cast_text          23  23     23  6 6 5 6
    parse_text         17  16     18  5 4 4 5
    float_special      24  24     24  6 6 6 6

    The minimum per (stratum, seed) is 2 (global_agg seed 3), per stratum 16 (global_agg)."""
    per_seed, total = {seed: 0 for seed in SEEDS}, 0
    for key in sorted(_keys_of(stratum), key=_rows_of_case):
        if total >= SENSITIVITY_PER_STRATUM and min(per_seed.values()) >= SENSITIVITY_PER_SEED:
            break
        if _detects(key, "far") or _detects(key, "near"):
            per_seed[key[1]] += 1
            total += 1
    assert min(per_seed.values()) >= SENSITIVITY_PER_SEED and total >= SENSITIVITY_PER_STRATUM, (stratum, per_seed, total)


def test_every_type_has_a_case_that_detects_its_poison_alone():
    """One column type unmasked at a time, over the cases of at most 9000 rows: for every type and each pool some case of the corpus detects.
    The count of detecting cases per (stratum, type), near / far, of the 22 cases of at most 9000 rows, from a full run:

    stratum          Int32     Int64     UInt64    Timestamp Float64   Utf8
    filter_project   10 / 12   0 / 0     0 / 0     10 / 10   5 / 5     6 / 8
    text             4 / 4     2 / 2     0 / 0     0 / 0     2 / 1     14 / 14
    group_narrow     11 / 11   7 / 7     4 / 4     3 / 3     4 / 4     0 / 0
    group_composite  12 / 12   3 / 3     7 / 7     7 / 8     6 / 6     13 / 13
    group_wide       13 / 13   17 / 17   11 / 12   13 / 13   8 / 8     3 / 3
    distinct_count   11 / 12   8 / 8     2 / 4     1 / 1     0 / 0     6 / 11
    global_agg       2 / 2     6 / 6     2 / 7     0 / 7     6 / 7     0 / 0
    join_inner       17 / 16   13 / 11   3 / 2     12 / 12   12 / 12   14 / 13
    join_semi_anti   3 / 3     20 / 18   0 / 0     0 / 0     0 / 0     16 / 16
    sort_limit       8 / 8     13 / 13   1 / 1     0 / 0     5 / 5     8 / 8
    window           18 / 18   15 / 15   7 / 8     3 / 4     6 / 6     0 / 0
    cross            11 / 11   10 / 12   0 / 0     7 / 7     8 / 8     10 / 10
    mixed            17 / 14   10 / 9    0 / 0     0 / 0     4 / 6     5 / 5
    union            17 / 18   14 / 15   5 / 5     1 / 1     2 / 2     20 / 20
    cast_text        16 / 16   16 / 16   9 / 9     12 / 12   2 / 2     8 / 8
    parse_text       3 / 3     4 / 4     4 / 4     4 / 4     0 / 0     13 / 10
    float_special    0 / 0     10 / 10   0 / 0     0 / 0     22 / 22   0 / 0

    A pair with 0 / 0 is a stratum whose plans read no column of that type, or none that holds a NULL; the corpus is not bent to fill them:
    filter_project x Int64, filter_project x UInt64, text x UInt64, text x Timestamp, group_narrow x Utf8, distinct_count x Float64,
    global_agg x Utf8, join_semi_anti x UInt64, join_semi_anti x Timestamp, join_semi_anti x Float64, sort_limit x Timestamp, window x Utf8,
    cross x UInt64, mixed x UInt64, mixed x Timestamp, parse_text x Float64, float_special x Int32, float_special x UInt64,
    float_special x Timestamp, float_special x Utf8."""
    for ty in POISON_TYPES:
        for pool in npz.POOLS:
            assert any(_detects(key, pool, ty) for s in NULL_STRATA for key in sorted(_keys_of(s), key=_rows_of_case) if _rows_of_case(key) <= 9000), (ty, pool)


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


def _batches(plan, tables, cuts_per_table, poison=None):
    """per leaf (in the interpreter's leaf order) the list of record batches: one batch, or one per pair of neighbouring cuts.  poison: None -- what
    pyarrow writes under a NULL (0, an empty range) --, or (pool, (stratum, seed, i)): what tests/null_poison.py puts there"""
    out = []
    for leaf, (fields, t, cuts) in enumerate(zip(pi.leaf_schemas(plan), tables, cuts_per_table)):
        n = len(t[fields[0]["name"]])
        cuts = cuts or [0, n]
        bs = []
        under = {f["name"]: npz.slots(poison[0], *poison[1], leaf, f["name"], t[f["name"]], f["data_type"]) for f in fields} if poison is not None else None
        for a, b in zip(cuts[:-1], cuts[1:]):
            arrs = []
            for f in fields:
                ty = _arrow(f["data_type"])
                if poison is not None:                           # (a row's poison does not depend on the cut)
                    arrs.append(npz.poisoned_array(under[f["name"]][a:b], [v is not None for v in t[f["name"]][a:b]], f["data_type"]))
                    continue
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
        _check_rows(key, schema, got, want, where)


def _check_rows(key, schema, got, want, where):
    """a result against the interpreter's: names and types where a batch came back, the rows (`want` normalised, and sorted where the case is not ordered)"""
    names, types, rows = _want(*key)
    if schema is not None:
        assert schema.names == names, where
        assert [f.type for f in schema] == [_arrow(t) for t in types], where
    else:
        assert not rows, where
    got = _norm(got)
    if not _case(*key).ordered:
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


# ------------------------------------------------------------------ GPU: what lies under a NULL
# Kernels of MUST_RUN that a near-poisoned whole feed may leave out, each with its reason.  Poison can legitimately change a route that depends on
# the DATA (uniqueness of a build side, strictly increasing keys); everything else that goes missing is a failure.
POISON_ROUTE_EXCEPTIONS = {
}


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("stratum", NULL_STRATA)
def test_gpu_ignores_what_lies_under_a_null(gpu, stratum, seed):
    """test_gpu_equals_the_interpreter with every NULL slot of every fed column holding tests/null_poison.py's values: every case fed whole, once
    with the near pool and once with the far pool, compared EXACTLY with the unchanged _want -- validity alone decides what is NULL.  That it would
    show is test_the_poison_would_change_the_answer_if_it_were_read.  Under near poison (which leaves every column's minimum and maximum where
    they were) the kernels of MUST_RUN must still run, POISON_ROUTE_EXCEPTIONS apart; under far poison what ran is printed."""
    from flock_amd.runtime import explain
    ran = {pool: set() for pool in npz.POOLS}
    for i in range(pc.CASES_PER_SEED):
        key = (stratum, seed, i)
        c = _case(*key)
        want = _norm(_want(*key)[2])
        if not c.ordered:
            want = _multiset(want)
        for pool in npz.POOLS:
            feeds = _batches(c.plan, c.tables, [None] * len(c.tables), poison=(pool, key))
            schema, got, r = _execute(gpu, c.plan, feeds, pc.generic_only(*key))
            ran[pool] |= r
            _check_rows(key, schema, got, want, "case%r %s poison (%s), generic_only=%s\n%s" % (key, pool, c.note, pc.generic_only(*key), explain(c.plan)))
    for pool in npz.POOLS:
        print("\n%s seed %d %s poison ran: %s" % (stratum, seed, pool, " ".join(sorted(ran[pool]))))
    excused = POISON_ROUTE_EXCEPTIONS.get(stratum, {})
    missing = [k for k in pc.MUST_RUN[stratum] if k not in excused and not any(name.startswith(k) for name in ran["near"])]
    assert not missing, (stratum, seed, missing, sorted(ran["near"]))


# ------------------------------------------------------------------ GPU: a failing value under a NULL fails nothing (literal plans and tables)
HOSTILE_ROWS = (65, 4097)
_TS0 = 1_436_918_400_000


def _hostile_cases():
    """name -> (columns, expression, its type, {column: value of live row k}, the column that holds the NULLs, what lies under them, {column: value
    beside a NULL row}, does a live row with that value fail the call).  `safe` in a name: the try_cast_expr form (a live row gives NULL there)."""
    out = {}
    ab32, ab64 = [("id", "Int64"), ("a", "Int32"), ("b", "Int32")], [("id", "Int64"), ("a", "Int64"), ("b", "Int64")]
    c = lambda cols, name: pc.col(name, cols)
    live_ab = {"a": lambda k: k * 3 - 100, "b": lambda k: k % 5 + 1}
    out["a / b over a zero divisor"] = (ab32, pc.binop(c(ab32, "a"), "Divide", c(ab32, "b")), "Int32", live_ab, "b", 0, {}, True)
    out["a % b over a zero divisor"] = (ab64, pc.binop(c(ab64, "a"), "Modulo", c(ab64, "b")), "Int64", live_ab, "b", 0, {}, True)
    out["INT_MIN under a NULL over -1"] = (ab32, pc.binop(c(ab32, "a"), "Divide", c(ab32, "b")), "Int32", live_ab, "a", -2**31, {"b": -1}, True)
    out["-1 under a NULL below INT_MIN"] = (ab32, pc.binop(c(ab32, "a"), "Divide", c(ab32, "b")), "Int32", live_ab, "b", -1, {"a": -2**31}, True)
    out["INT64_MIN % -1 under a NULL"] = (ab64, pc.binop(c(ab64, "a"), "Modulo", c(ab64, "b")), "Int64", live_ab, "b", -1, {"a": -2**63}, True)
    for safe in (False, True):
        tag = " (safe)" if safe else ""
        cols = [("id", "Int64"), ("l", "Int64")]
        out["Int64 to Int32 over 2^40" + tag] = (cols, pc.cast(c(cols, "l"), "Int32", safe), "Int32", {"l": lambda k: k * 1000 - 5}, "l", 2**40, {}, not safe)
        cols = [("id", "Int64"), ("f", "Float64")]
        for what, v in (("NaN", float("nan")), ("1e300", 1e300)):
            out["Float64 to Int64 over %s%s" % (what, tag)] = (cols, pc.cast(c(cols, "f"), "Int64", safe), "Int64", {"f": lambda k: k / 4 - 9}, "f", v, {}, not safe)
        cols = [("id", "Int64"), ("s", "Utf8")]
        for ty in ("Int32", "Int64", "UInt64"):
            out["Utf8 to %s over '12x'%s" % (ty, tag)] = (cols, pc.cast(c(cols, "s"), ty, safe), ty, {"s": lambda k: str(k * 7)}, "s", b"12x", {}, not safe)
        out["Utf8 to Timestamp over '12x'" + tag] = (cols, pc.cast(c(cols, "s"), "ts", safe), "ts", {"s": lambda k: "2015-03-%02d" % (k % 28 + 1)}, "s", b"12x", {}, not safe)
        cols = [("id", "Int64"), ("t", "ts")]
        out["Timestamp to Utf8 over the year 10000" + tag] = (cols, pc.cast(c(cols, "t"), "Utf8", safe), "Utf8", {"t": lambda k: _TS0 + 86_399_123 * k}, "t", pc.TS_MAX + 1, {}, not safe)
    # no status of the dialect: sqrt of a negative is NaN, date_trunc has no range check (and Python's datetime ends before INT64_MIN: nothing to expect
    # of a live row) -- the NULL rows must still come out NULL, whatever the slot would have given
    cols = [("id", "Int64"), ("f", "Float64")]
    out["sqrt over -1"] = (cols, pc.fn("sqrt", "Float64", c(cols, "f")), "Float64", {"f": lambda k: k / 4}, "f", -1.0, {}, False)
    cols = [("id", "Int64"), ("t", "ts")]
    out["date_trunc over INT64_MIN"] = (cols, pc.fn("date_trunc", "ts", pc.lit("Utf8", "month"), c(cols, "t")), "ts", {"t": lambda k: _TS0 + 86_399_123 * k}, "t", -2**63, {}, None)
    return out


HOSTILE = _hostile_cases()


def _hostile_rows(n):
    return sorted({k for k in range(n) if k % 7 == 3} | {k for k in (0, 63, 64, 4095, 4096, n - 1) if k < n})


def _hostile_tables(name, n):
    """-> (the table with None in the NULL rows, the same with what lies under them as live values, per column its slots)"""
    cols, _, _, live, null_col, slot, beside, _ = HOSTILE[name]
    at = set(_hostile_rows(n))
    masked, unmasked = {"id": list(range(n))}, {"id": list(range(n))}
    for col, make in live.items():
        vals = [beside[col] if (k in at and col in beside) else make(k) for k in range(n)]
        masked[col] = [None if (k in at and col == null_col) else v for k, v in enumerate(vals)]
        unmasked[col] = [slot if (k in at and col == null_col) else v for k, v in enumerate(vals)]
    return masked, unmasked


def _hostile_plans(name):
    """the expression as a projected column, and as a filter's predicate (IS NOT NULL of it: a computed leaf, the general evaluator)"""
    cols, e, ty, _, _, _, _, _ = HOSTILE[name]
    a = pc.scan(cols)
    return {"projection": pc.proj(a, [(a.c("id"), "id", "Int64"), (e, "e", ty)]).plan,
            "filter": pc.keep(pc.filt(a, {"physical_expr": "is_not_null_expr", "arg": e}), ["id"]).plan}


def _hostile_batch(name, n, all_valid):
    """the record batch: the slots hold the unmasked table's values, the validity is the masked table's (or all 1)"""
    cols = HOSTILE[name][0]
    masked, unmasked = _hostile_tables(name, n)
    arrs = []
    for col, ty in cols:
        slots = [v.encode() if isinstance(v, str) else v for v in unmasked[col]]
        arrs.append(npz.poisoned_array(slots, [all_valid or v is not None for v in masked[col]], ty))
    return [[pa.record_batch(arrs, names=[col for col, _ in cols])]]


def _as_text(table):
    return {k: [v.decode() if isinstance(v, bytes) else v for v in vals] for k, vals in table.items()}


@pytest.mark.parametrize("name", sorted(HOSTILE))
def test_the_hostile_slots_are_hostile_to_the_interpreter(name):
    """CPU: over the masked table every plan evaluates (NULL in, NULL out); with the slots as live values the interpreter raises ExprError exactly
    where the case says a live row fails -- and, for sqrt, another result (NaN is a value)"""
    from flock_amd.runtime import explain
    fails = HOSTILE[name][7]
    for n in HOSTILE_ROWS[:1]:
        masked, unmasked = _hostile_tables(name, n)
        for how, plan in _hostile_plans(name).items():
            explain(plan)
            rows = run_plan(plan, [masked])[2]
            assert len(rows) == (n if how == "projection" else n - len(_hostile_rows(n))), (name, how)
            if how == "projection":
                assert [r[1] is None for r in rows] == [k in set(_hostile_rows(n)) for k in range(n)], name
            if fails:
                with pytest.raises(g.ExprError):
                    run_plan(plan, [_as_text(unmasked)])
            elif name == "sqrt over -1":                         # (a safe cast of a live row gives the NULL the NULL row gives: only the GPU run can tell)
                assert _norm(run_plan(plan, [_as_text(unmasked)])[2]) != _norm(rows), (name, how)


@pytest.mark.gpu
@pytest.mark.parametrize("n", HOSTILE_ROWS)
@pytest.mark.parametrize("name", sorted(HOSTILE))
def test_a_failing_value_under_a_null_fails_nothing(gpu, name, n):
    """Every NULL row's slot holds what would fail a live row (a zero divisor, INT_MIN over -1, a value that does not fit the cast, a text that does
    not parse, a timestamp in the year 10000): as a projected column and under a filter's predicate the call succeeds and equals the interpreter.
    The same slots with validity all 1 fail the call with FLOCKGPU_ERR_INVALID, as the `errors` strata do -- the slot really is hostile; where the
    dialect has no status for the value (a safe cast, sqrt of a negative) the all-valid run equals the interpreter over the unmasked table.
    CAST(Timestamp AS Utf8) under a predicate is outside the dialect: the filter form of that case is refused by name, with and without NULLs."""
    from flock_amd import FlockGpuError, _ffi
    fails = HOSTILE[name][7]
    masked, unmasked = _hostile_tables(name, n)
    one_nan = lambda rows: [tuple("NaN" if isinstance(v, float) and v != v else v for v in r) for r in rows]      # (the sign of sqrt(-1)'s NaN is the machine's)
    for how, plan in _hostile_plans(name).items():
        want = _norm(run_plan(plan, [masked])[2])
        if how == "filter" and HOSTILE[name][2] == "Utf8":
            # a text-valued CAST under a predicate is outside the dialect (the general evaluator takes no text): refused by name, NULLs or not
            for all_valid in (False, True):
                with pytest.raises(FlockGpuError) as e:
                    _execute(gpu, plan, _hostile_batch(name, n, all_valid), True)
                assert e.value.code == _ffi.ERR_UNSUPPORTED and "CAST" in str(e.value), (name, str(e.value))
            continue
        _, got, ran = _execute(gpu, plan, _hostile_batch(name, n, False), True)
        assert _norm(got) == want, (name, how, n, sorted(ran))
        if fails:
            with pytest.raises(FlockGpuError) as e:
                _execute(gpu, plan, _hostile_batch(name, n, True), True)
            assert e.value.code == _ffi.ERR_INVALID, (name, how, str(e.value))
        elif fails is False:
            _, got, _ = _execute(gpu, plan, _hostile_batch(name, n, True), True)
            assert _norm(one_nan(got)) == _norm(one_nan(run_plan(plan, [_as_text(unmasked)])[2])), (name, how, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", HOSTILE_ROWS)
def test_a_matching_value_under_a_null_selects_nothing_in_the_one_pass_predicate(gpu, n):
    """the leaves of the one-pass predicate program (a column or its remainder against a literal, IN, LIKE, a Utf8 comparison) cannot fail, but they
    can MATCH: every NULL row's slot satisfies its leaf, and no NULL row is selected.  With validity all 1 every such row is."""
    cols = [("id", "Int64"), ("i", "Int32"), ("l", "Int64"), ("s", "Utf8"), ("f", "Float64")]
    a = pc.scan(cols)
    at = set(_hostile_rows(n))
    slots = {"id": list(range(n)), "i": [6 if k in at else 1 for k in range(n)], "l": [2**40 if k in at else 5 for k in range(n)],
             "s": [b"12x" if k in at else b"no" for k in range(n)], "f": [float("inf") if k in at else 0.25 for k in range(n)]}
    leaves = {"i": pc.binop(a.c("i"), "Eq", pc.lit("Int32", 6)), "i%": pc.binop(pc.binop(a.c("i"), "Modulo", pc.lit("Int32", 3)), "Eq", pc.lit("Int32", 0)),
              "i in": {"physical_expr": "in_list_expr", "expr": a.c("i"), "list": [pc.lit("Int32", x) for x in (6, 7, 8)], "negated": False},
              "l": pc.binop(a.c("l"), "Gt", pc.lit("Int64", 100)), "s like": pc.binop(a.c("s"), "Like", pc.lit("Utf8", "1%x")),
              "s not like": pc.binop(a.c("s"), "NotLike", pc.lit("Utf8", "n_")), "s cmp": pc.binop(a.c("s"), "Lt", pc.lit("Utf8", "2")),
              "f": pc.binop(a.c("f"), "Gt", pc.lit("Float64", 3.0))}
    for what, pred in leaves.items():
        plan = pc.keep(pc.filt(a, pred), ["id"]).plan
        col = what.split()[0].rstrip("%")
        for all_valid in (False, True):
            arrs = [npz.poisoned_array(slots[c], [all_valid or c != col or k not in at for k in range(n)], ty) for c, ty in cols]
            _, got, ran = _execute(gpu, plan, [[pa.record_batch(arrs, names=[c for c, _ in cols])]], True)
            assert sorted(r[0] for r in got) == (sorted(at) if all_valid else []), (what, n, all_valid)
            assert "pred_flag_kernel" in ran or any(k.startswith("strmatch") for k in ran), (what, sorted(ran))
            table = {c: [None if (not all_valid and c == col and k in at) else (v.decode() if isinstance(v, bytes) else v) for k, v in enumerate(slots[c])] for c, _ in cols}
            assert sorted(r[0] for r in run_plan(plan, [table])[2]) == sorted(r[0] for r in got), what


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
