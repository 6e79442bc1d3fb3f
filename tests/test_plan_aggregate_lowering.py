"""One lowering of a node's aggregates, three back-ends (flock_amd/csrc/plan.hip lower_aggregates): the ungrouped pass (reduce.hpp), the GROUP BY tables
of at most four accumulators (relops.hpp) and the one pass over group ids of five to sixteen (groupwide.hpp).  The same rows go through all three -- the
grouped node as it stands and padded with COUNT(*) entries to five accumulators, the ungrouped node beside a one-group key -- and the results must be equal
bit for bit, to each other and to the references (tests/wide_group_ref.py grouped, tests/global_agg_ref.py ungrouped).

Every function (COUNT, SUM, MIN, MAX, AVG, distinct_count) x {single pass, Partial, Partial -> Final} x {Int32, Int64, UInt64, Timestamp, Float64 (COUNT / MIN /
MAX)} x {no NULLs, some NULLs, one group nothing but NULLs}.  A node is finished in a single pass exactly when it carries a distinct count, so that mode
is every list beside one.  Final mode reads the states of two Partials, each over half the rows, from a scan: a Final directly over its own Partial
is a shortcut that aggregates nothing.

Values keep every integer sum below 2^53 (asserted on the inputs): (double) sum / (double) count is then the same IEEE division in every back-end and in
both references, whichever way a back-end converts a UInt64 sum.

Refusals: each at the stage -- create or execute -- that makes it, in its words.  One difference between the back-ends has no test here because no plan
reaches it: the grouped paths refuse an argument that is all NULL and not materialised ("... needs an integer column") where the ungrouped pass takes it.
A column is unmaterialised only when no operator above reads it, and the one place that marks a column all-NULL, the lone integer MAX over no value,
materialises its one row: an aggregate's argument is never both."""
import numpy as np
import pytest

import global_agg_ref as gref
import test_plan_wide_group_by as wg
import wide_group_ref as ref

TILE = wg.TILE
ROWS = TILE + 5                       # just over one tile of the wide pass (and of the ungrouped pass's flag tiles)
MANY = wg.BINS[8] + 12                # groups above the wide pass's LDS bins for five to eight accumulators (and so above those for nine to sixteen)
# keys: k1 one group, kd dense Int32, kp Int32 (pairs with kd), kw Int64 spread over 2^40, ks Utf8, kn Int32 with NULL keys, k2 Int64 with NULL keys;
# arguments i l u t f; d: the distinct count's
COLS = [("k1", "Int32"), ("kd", "Int32"), ("kp", "Int32"), ("kw", "Int64"), ("ks", "Utf8"), ("kn", "Int32"), ("k2", "Int64"),
        ("i", "Int32"), ("l", "Int64"), ("u", "UInt64"), ("t", "ts"), ("f", "Float64"), ("d", "Int32")]
TYPES = dict(COLS)
INTS = ["i", "l", "u", "t"]
# every (function, argument type) in lists of at most four accumulators (AVG takes two)
LISTS = [[("sum", "i"), ("min", "l"), ("max", "u"), ("count", "t")],
         [("avg", "i"), ("min", "f"), ("count", "f")],
         [("avg", "l"), ("max", "f"), ("count", "i")],
         [("avg", "u"), ("min", "i"), ("max", "i")],
         [("avg", "t"), ("sum", "l"), ("count", "l")],
         [("sum", "u"), ("sum", "t"), ("min", "u"), ("max", "l")],
         [("min", "t"), ("max", "t"), ("count", "u"), ("count", None)]]
assert {a for l in LISTS for a in l} >= {(fn, c) for c in INTS + ["f"] for fn in ("count", "sum", "min", "max", "avg") if c != "f" or fn in ("count", "min", "max")}
assert all(wg.n_accs(l) <= 4 for l in LISTS)
DC = ("dc", "d")
KEYS = {"dense_i32": ["kd"], "spread_i64": ["kw"], "utf8": ["ks"], "pair_i32": ["kd", "kp"], "composite": ["ks", "kd", "kw"], "null_i32": ["kn"], "null_i64": ["k2"]}


def padded(aggs):
    """the same list with COUNT(*) entries behind it, to five accumulators: the path of groupwide.hpp"""
    return aggs + [("count", None)] * (5 - wg.n_accs(aggs))


# ------------------------------------------------------------------ tables
_tables = {}


def table(n, groups, nulls):
    """nulls: "none"; "some" a quarter of every argument; "group" the same, and group 0 holds nothing but NULLs in every argument (with one group: the
    whole column).  Built once per shape, shared, never changed."""
    key = (n, groups, nulls)
    if key in _tables:
        return _tables[key]
    r = np.random.default_rng(1000 + n + 7 * groups + len(nulls))
    g = np.arange(n, dtype=np.int64) % groups if groups > 7 else r.integers(0, groups, n).astype(np.int64)   # (many groups: every tile spans all ids)
    t = {"k1": [5] * n, "kd": (g + 100).tolist(), "kp": (g % 3).tolist(), "kw": ((g * 0x9E3779B1) % (1 << 40) - (1 << 39)).tolist(),
         "ks": ["key-%d" % k if k else "" for k in g.tolist()], "kn": [None if k == 1 else k for k in g.tolist()],
         "k2": [None if k % 5 == 2 else k // 5 * 10**12 for k in g.tolist()],
         "i": r.integers(-2**31, 2**31, n).tolist(), "l": r.integers(-10**11, 10**11, n).tolist(), "u": r.integers(0, 2**39, n).tolist(),
         "t": (10**9 + r.integers(0, 10**9, n)).tolist(), "f": [[-0.0, 0.0, -1.5][int(v)] if v < 3 else float(v - 40) * 0.37 for v in r.integers(0, 80, n).tolist()],
         "d": r.integers(0, 40, n).tolist()}
    if nulls != "none":
        for c in INTS + ["f", "d"]:
            ok = r.random(n) >= 0.25
            t[c] = [v if o and not (nulls == "group" and k == 0) else None for v, o, k in zip(t[c], ok.tolist(), g.tolist())]
    # the bound under which AVG is one exact IEEE division everywhere: every integer sum -- of a group, of a half, of the whole -- below 2^53
    for c in INTS:
        assert sum(abs(v) for v in t[c] if v is not None) < 2**53, c
    _tables[key] = t
    return t


def as_columns(t):
    """the ungrouped reference's table: {name: (values, valid)}"""
    dt = {"UInt64": np.uint64, "Float64": np.float64}
    return {c: (np.array([0 if v is None else v for v in t[c]], dt.get(TYPES[c], np.int64)), np.array([v is not None for v in t[c]], bool)) for c in INTS + ["f", "d"]}


@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


# ------------------------------------------------------------------ plans and what they must return
def whole(keys, aggs):
    if keys:
        return wg.whole_plan(keys, aggs, cols=COLS)
    part = wg.agg_node("Partial", [], aggs, wg._scan(COLS), COLS)
    return wg.agg_node("Final", [], aggs, {"execution_plan": "coalesce_partitions_exec", "input": part}, COLS)


def flat_states(aggs):
    """a Partial's state columns as aggregates: AVG -> (count, sum); and the places of the sums, which are Float64 there (0.0 over no value)"""
    flat, sums = [], []
    for fn, arg in aggs:
        if fn == "avg":
            sums.append(len(flat) + 1)
            flat += [("count", arg), ("sum", arg)]
        else:
            flat.append((fn, arg))
    return flat, sums


def got_rows(gpu, t, keys, aggs, mode):
    """the node's rows over t, sorted by key: mode "single" (aggs carries the distinct count), "partial" (the state columns), "final" """
    feed = wg.batches(t, 2, COLS)
    if mode == "single":
        out = wg.run(gpu, whole(keys, aggs), [feed])
    elif mode == "partial":
        out = wg.run(gpu, wg.agg_node("Partial", keys, aggs, wg._scan(COLS), COLS), [feed])
    else:
        scols = [(k, TYPES[k]) for k in keys] + wg.state_cols(aggs, COLS)
        halves = [s for b in feed for s in wg.run(gpu, wg.agg_node("Partial", keys, aggs, wg._scan(COLS), COLS), [[b]])]
        halves = halves or [wg.record_batch({c: [] for c, _ in scols}, cols=scols)]      # (GROUP BY over no rows returns no batch)
        out = wg.run(gpu, wg.agg_node("Final" if not keys else "FinalPartitioned", keys, aggs, wg._scan(scols), COLS), [halves])
    return ref.sort_rows(wg.out_rows(out), len(keys))


def want_grouped(t, keys, aggs, mode):
    """wide_group_ref's rows; a distinct count beside them is the size of a set"""
    flat, sums = flat_states(aggs) if mode == "partial" else (aggs, [])
    plain = [a for a in flat if a != DC]
    rows = ref.aggregate(t, keys, plain, TYPES)
    n_dc = {}
    for r in range(len(t["d"])):
        n_dc.setdefault(tuple(t[k][r] for k in keys), set()).add(t["d"][r])
    out = []
    for row in rows:
        key, vals = row[:len(keys)], list(row[len(keys):])
        for s in sums:
            vals[s] = float(vals[s] or 0)
        for at, a in enumerate(flat):
            if a == DC:
                vals.insert(at, len(n_dc[key] - {None}))
        out.append(tuple(key) + tuple(vals))
    return ref.sort_rows(out, len(keys))


def want_ungrouped(t, aggs, mode):
    """global_agg_ref's one row"""
    cols = as_columns(t)
    if mode == "partial":
        return tuple(gref.partial_state(cols, aggs))
    row = gref.reference_row(cols, [a for a in aggs if a != DC])
    for at, a in enumerate(aggs):
        if a == DC:
            row.insert(at, len(set(t["d"]) - {None}))
    return tuple(row)


def three_ways(gpu, t, keys, aggs, mode, ungrouped=False):
    """narrow and wide over `keys`, equal to each other and to the reference; `ungrouped`: keys is a one-group key and the node without it agrees too"""
    nk, pad = len(keys), 5 - wg.n_accs(aggs)
    last = [DC] if mode == "single" else []
    want = want_grouped(t, keys, aggs + last, mode)
    narrow = got_rows(gpu, t, keys, aggs + last, mode)
    wide = got_rows(gpu, t, keys, padded(aggs) + last, mode)
    # the wide node's columns: keys, the shared results, the COUNT(*) entries, the distinct count
    cut = nk + len(flat_states(aggs)[0] if mode == "partial" else aggs)
    shared = [r[:cut] + r[cut + pad:] for r in wide]
    assert pad > 0 and all(len(r) == len(want[0]) + pad for r in wide)
    assert ref.same_rows(narrow, shared), (keys, aggs, mode, [p for p in zip(narrow, shared) if p[0] != p[1]][:3])
    assert ref.same_rows(narrow, want), (keys, aggs, mode, [p for p in zip(narrow, want) if p[0] != p[1]][:3])
    sizes = {r[:nk]: r[nk] for r in ref.aggregate(t, keys, [("count", None)], TYPES)}
    assert all(list(r[cut:cut + pad]) == [sizes[r[:nk]]] * pad for r in wide)       # every COUNT(*) is the group's rows
    if ungrouped:
        alone = got_rows(gpu, t, [], aggs + last, mode)
        assert ref.same_rows(alone, [want_ungrouped(t, aggs + last, mode)]), (aggs, mode, alone)
        if narrow:    # (over no rows GROUP BY returns no group, the ungrouped node its one row)
            assert len(narrow) == 1 and ref.same_rows(alone, [narrow[0][nk:]]), (aggs, mode, alone, narrow)
    return narrow


# ------------------------------------------------------------------ CPU: the references agree with each other where both apply
def test_the_two_references_agree_over_one_group():
    t = table(ROWS, 1, "some")
    for aggs in LISTS:
        one, = ref.aggregate(t, ["k1"], aggs, TYPES)
        assert ref.same_rows([one[1:]], [tuple(gref.reference_row(as_columns(t), aggs))]), aggs


# ------------------------------------------------------------------ CPU: refusals, each at the stage that has made it so far
def _refused(plan, words):
    from flock_amd import FlockGpuError
    from flock_amd.runtime import explain
    with pytest.raises(FlockGpuError) as e:
        explain(plan)
    assert words in str(e.value), (words, str(e.value))


def test_create_time_refusals_keep_their_words():
    ungrouped = lambda aggs: wg.agg_node("Partial", [], aggs, wg._scan(COLS), COLS)
    _refused(ungrouped([("sum", "f")]), "sum needs an integer column")
    _refused(ungrouped([("avg", "f")]), "avg needs an integer column")             # (lower case at create)
    _refused(ungrouped([("max", "ks")]), "max needs an integer column")
    _refused(ungrouped([("count", "ks")]), "count needs an integer column")        # (COUNT of a Utf8 column: the ungrouped pass alone refuses it)
    _refused(whole(["kd"], [("dc", "f")]), "distinct_count needs an integer or Utf8 column")
    _refused(whole([], [("dc", "f")]), "distinct_count needs an integer or Utf8 column")
    # the limits: 16 grouped, 8 ungrouped, 4 distinct counts
    _refused(whole(["kd"], [("avg", c) for c in INTS] * 2 + [("count", None)]), "more than 16 accumulators in one GROUP BY")
    _refused(ungrouped([("avg", c) for c in INTS] + [("count", None)]), "more than 8 accumulators in one ungrouped aggregate")
    _refused(whole(["kd"], [("dc", c) for c in INTS + ["d"]]), "more than 4 distinct counts")


def test_what_create_lets_through_for_execute_to_refuse():
    """SUM / AVG of Float64 and COUNT of Utf8 under GROUP BY explain: the first two are refused at execute (test_execute_time_refusals...), the last runs"""
    from flock_amd.runtime import explain
    for aggs in ([("sum", "f")], [("avg", "f")], [("count", "ks")], padded([("avg", "f")])):
        assert explain(whole(["kd"], aggs)).startswith("Aggregate(")
    assert explain(whole(["kd"], [("avg", c) for c in INTS] * 2)).startswith("Aggregate(")             # sixteen
    assert explain(whole([], [("avg", c) for c in INTS])).startswith("Aggregate(")                     # eight
    assert "single pass" in explain(whole([], [("dc", c) for c in INTS] + [("count", None)]))           # four distinct counts


# a Final whose first aggregate's state column `suffix` arrives as type `ty`, and the words it is refused with at execute
BAD_STATES = [([("count", "i")], "[count]", "Float64", "the COUNT state needs an integer column"),
              ([("avg", "i")], "[count]", "Float64", "the AVG count state needs an integer column"),
              ([("avg", "i")], "[sum]", "Int64", "the AVG sum state must be Float64")]


def final_over(keys, aggs, suffix, ty):
    """-> (a Final of `aggs` over a scan of its state columns, those columns), the first column that ends in `suffix` retyped"""
    states = wg.state_cols(aggs, COLS)
    at = [n.endswith(suffix) for n, _ in states].index(True)
    states[at] = (states[at][0], ty)
    scols = [(k, TYPES[k]) for k in keys] + states
    return wg.agg_node("FinalPartitioned" if keys else "Final", keys, aggs, wg._scan(scols), COLS), scols


def test_state_columns_of_the_wrong_type_at_create():
    """Create checks no state column's type under GROUP BY; without GROUP BY it holds a Final's first state column to the function's argument rule, in
    create's words.  The rest is execute's (test_state_columns_of_the_wrong_type_are_refused_at_execute)."""
    from flock_amd.runtime import explain
    for aggs, suffix, ty, words in BAD_STATES:
        assert explain(final_over(["kd"], aggs, suffix, ty)[0]).startswith("Aggregate(")
        if words == "the AVG count state needs an integer column":
            _refused(final_over([], aggs, suffix, ty)[0], "avg needs an integer column")
        else:
            assert explain(final_over([], aggs, suffix, ty)[0]).startswith("Aggregate(")


# ------------------------------------------------------------------ GPU 1: the matrix
@pytest.mark.gpu
@pytest.mark.parametrize("groups", [1, 7])
@pytest.mark.parametrize("nulls", ["none", "some", "group"])
@pytest.mark.parametrize("mode", ["single", "partial", "final"])
def test_every_function_type_and_null_pattern_three_ways(gpu, mode, nulls, groups):
    t = table(ROWS, groups, nulls)
    for aggs in LISTS:
        got = three_ways(gpu, t, ["k1" if groups == 1 else "kd"], aggs, mode, ungrouped=groups == 1)
        assert len(got) == groups


# ------------------------------------------------------------------ GPU 2: sizes
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1])
@pytest.mark.parametrize("mode", ["single", "partial", "final"])
def test_no_row_and_one_row(gpu, mode, n):
    for nulls in ("none", "group"):       # (one row: a value, a NULL)
        for aggs in LISTS:
            assert len(three_ways(gpu, table(n, 1, nulls), ["k1"], aggs, mode, ungrouped=True)) == n


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["single", "partial", "final"])
def test_more_groups_than_the_wide_pass_has_lds_bins(gpu, mode):
    assert MANY > wg.BINS[8] >= wg.BINS[16]
    for aggs in LISTS:
        assert len(three_ways(gpu, table(ROWS, MANY, "group"), ["kd"], aggs, mode)) == MANY


# ------------------------------------------------------------------ GPU 3: key shapes (Partial and Final: a single-pass node groups on composite ids whatever its key)
@pytest.mark.gpu
@pytest.mark.parametrize("mode,nulls", [("partial", "none"), ("partial", "some"), ("final", "some")])
@pytest.mark.parametrize("shape", sorted(KEYS))
def test_every_key_shape_with_every_list(gpu, shape, mode, nulls):
    """("none": accumulators without validity, under which a dense Int32 key and a Utf8 key's codes take the direct-address table)"""
    t = table(ROWS, 7, nulls)
    for aggs in LISTS:
        got = three_ways(gpu, t, KEYS[shape], aggs, mode)
        if shape.startswith("null"):
            assert got[0][0] is None      # NULL keys form one group


# ------------------------------------------------------------------ GPU 4: execute-time refusals
def _refused_at_execute(gpu, plan, feed, words):
    from flock_amd import FlockGpuError
    with pytest.raises(FlockGpuError) as e:
        wg.run(gpu, plan, [feed])
    assert words in str(e.value), (words, str(e.value))


@pytest.mark.gpu
def test_execute_time_refusals_keep_their_words(gpu):
    feed = wg.batches(table(1, 1, "none"), 1, COLS)
    for fn, words in (("sum", "sum needs an integer column"), ("avg", "AVG needs an integer column")):   # (upper case at execute)
        for aggs in ([(fn, "f")], padded([(fn, "f")])):
            _refused_at_execute(gpu, whole(["kd"], aggs), feed, words)


@pytest.mark.gpu
def test_a_ninth_key_column_is_refused_at_execute(gpu):
    keys = ["kd", "kp", "kw", "ks", "kn", "k2", "k1", "i", "l"]
    feed = wg.batches(table(1, 1, "none"), 1, COLS)
    for aggs in (LISTS[0], padded(LISTS[0])):
        _refused_at_execute(gpu, wg.agg_node("Partial", keys, aggs, wg._scan(COLS), COLS), feed, "GROUP BY more than 8 columns")
    assert len(wg.run(gpu, wg.agg_node("Partial", keys[:8], LISTS[0], wg._scan(COLS), COLS), [feed])[0]) == 1      # eight run


@pytest.mark.gpu
@pytest.mark.parametrize("keys", [[], ["kd"]], ids=["ungrouped", "grouped"])
def test_state_columns_of_the_wrong_type_are_refused_at_execute(gpu, keys):
    for aggs, suffix, ty, words in BAD_STATES:
        if not keys and words == "the AVG count state needs an integer column":
            continue      # (without GROUP BY create has refused it: test_state_columns_of_the_wrong_type_at_create)
        for mine in ((aggs,) if not keys else (aggs, padded(aggs))):
            plan, scols = final_over(keys, mine, suffix, ty)
            row = {c: ["x" if t == "Utf8" else 1.0 if t == "Float64" else 1] for c, t in scols}
            _refused_at_execute(gpu, plan, [wg.record_batch(row, cols=scols)], words)
