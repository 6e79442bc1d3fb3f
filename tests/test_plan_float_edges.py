"""Float64 special values -- NaNs of four patterns, both zeros, both infinities, subnormals, +-DBL_MAX, the edges of the integer types -- through the
kernels that ORDER, COMPARE and CONVERT doubles: the sort (A-FO1 of relops.hpp), the window's partition and peer tests and ROW_NUMBER's runs (A-FO2),
the one-pass predicate program and the general evaluator (A-FO3), CAST / TRY_CAST (A-V5 of valprog.hpp).  Every plan runs through the plan ABI
(ExecutionContext + collect), every comparison is exact, Float64 by its bits; what is expected comes from tests/float_order_ref.py, numpy's IEEE
comparison of the same bits, oracle.generic_ops' typed evaluator, the interpreter of tests/plan_interp.py, or is written out by hand.

Arrays are built from their BUFFERS (a uint64 buffer read as Float64), so nothing between Python and the device quiets a signalling NaN, and the
slot of a NULL holds the bits the test puts there.

The CPU tests pin the references themselves: float_order_ref against hand-written orderings, numpy and pyarrow (ascending with NULLs last; descending
on NaN-free columns only: pyarrow keeps NaNs with the NULLs, Arrow C++'s rule and not arrow-rs'), the bit-exact round trip, generic_ops' cast."""
import itertools
import math

import numpy as np
import pyarrow as pa
import pyarrow.compute as pac
import pytest

import float_order_ref as fo
import plan_corpus as pc
from oracle import generic_ops as g
from plan_interp import run_plan
from test_plan_differential import _execute, _norm

F = fo.from_bits
POOL = [F(b) for b in fo.SPECIALS]
OPTIONS = [(False, False), (False, True), (True, False), (True, True)]          # (descending, nulls_first)
NP_CMP = {"Eq": np.equal, "NotEq": np.not_equal, "Lt": np.less, "LtEq": np.less_equal, "Gt": np.greater, "GtEq": np.greater_equal}
PY_CMP = {"Eq": lambda a, b: a == b, "NotEq": lambda a, b: a != b, "Lt": lambda a, b: a < b, "LtEq": lambda a, b: a <= b, "Gt": lambda a, b: a > b,
          "GtEq": lambda a, b: a >= b}
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64()}


# ------------------------------------------------------------------ arrays by their buffers
def f64_array(values, slots=None):
    """a Float64 array of Python floats / None: the value buffer is the floats' bits, the slot of NULL row k holds slots[k] (0 when not named)"""
    slots = slots or {}
    u = np.array([slots.get(k, 0) if v is None else fo.bits(v) for k, v in enumerate(values)], dtype=np.uint64)
    live = np.array([v is not None for v in values], dtype=bool)
    validity = None if live.all() else pa.py_buffer(np.packbits(live, bitorder="little").tobytes())
    return pa.Array.from_buffers(pa.float64(), len(values), [validity, pa.py_buffer(u.tobytes())], int((~live).sum()))


def batch(cols, t, lo=0, hi=None, slots=None):
    """cols: [(name, type)]; t: {name: [values]}; slots: {name: {row: bits}} for the slots of NULL Float64 rows"""
    hi = len(t[cols[0][0]]) if hi is None else hi
    arrs = []
    for name, ty in cols:
        if ty == "Float64":
            arrs.append(f64_array(t[name][lo:hi], {k - lo: b for k, b in (slots or {}).get(name, {}).items() if lo <= k < hi}))
        else:
            arrs.append(pa.array(t[name][lo:hi], _PA[ty]))
    return pa.record_batch(arrs, names=[n for n, _ in cols])


def run(gpu, node, cols, t, cuts=None, slots=None, must_run=()):
    """the plan's rows over table t (one leaf), by bits; cuts: batch boundaries"""
    cuts = cuts or [0, len(t[cols[0][0]])]
    feeds = [[batch(cols, t, a, b, slots) for a, b in zip(cuts[:-1], cuts[1:])]]
    _, rows, ran = _execute(gpu, node.plan, feeds, True)
    missing = [k for k in must_run if not any(name.startswith(k) for name in ran)]
    assert not missing, (missing, sorted(ran))
    return _norm(rows)


def want(node, t):
    return _norm(run_plan(node.plan, [t])[2])


@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


# ------------------------------------------------------------------ CPU: the reference of the rule
def test_the_pool_is_what_it_says():
    assert len(set(fo.SPECIALS)) == len(fo.SPECIALS) == 20 and len(fo.NAN_FREE) == 16
    assert [math.isnan(x) for x in POOL] == [True] * 4 + [False] * 16
    named = [0.0, -0.0, math.inf, -math.inf, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 2.225073858507201e-308, -2.225073858507201e-308,
             1.7976931348623157e308, -1.7976931348623157e308, 1.0, -1.0, 2.0**53, 2.0**53 + 2]
    assert [fo.bits(x) for x in named] == fo.SPECIALS[4:]
    assert all(fo.bits(F(b)) == b for b in fo.SPECIALS)                    # Python floats keep every pattern, the signalling NaN included


def test_key_against_hand_written_orderings():
    nan, nnan, snan, ones = POOL[:4]
    asc = [-math.inf, -1.7976931348623157e308, -1.0, -2.2250738585072014e-308, -2.225073858507201e-308, -5e-324, 0.0, 5e-324, 2.225073858507201e-308,
           2.2250738585072014e-308, 1.0, 2.0**53, 2.0**53 + 2, 1.7976931348623157e308, math.inf, nan]
    assert all(fo.key(a) < fo.key(b) for a, b in zip(asc, asc[1:]))
    assert fo.key(-0.0) == fo.key(0.0) and fo.same(-0.0, 0.0) and not fo.same(0.0, 5e-324) and not fo.same(-5e-324, 0.0)
    assert len({fo.key(x) for x in (nan, nnan, snan, ones)}) == 1 and all(fo.same(a, b) for a in POOL[:4] for b in POOL[:4])
    assert fo.key(nnan) > fo.key(math.inf) and fo.key(ones) > fo.key(math.inf)          # a NaN with the sign bit set is last, too
    # ties keep input order; DESC is the reverse on values with ties still in input order
    col = [nnan, 0.0, math.inf, -0.0, snan, -math.inf, 0.0, nan]
    up = sorted(range(8), key=lambda i: fo.key(col[i]))
    down = sorted(range(8), key=lambda i: fo.key(col[i]), reverse=True)
    assert up == [5, 1, 3, 6, 2, 0, 4, 7] and down == [0, 4, 7, 2, 1, 3, 6, 5]
    # A-FO4: the order of the order keys -- the zeros differ, and the key is total
    assert fo.total_key(-0.0) < fo.total_key(0.0) and fo.total_key(-5e-324) < fo.total_key(-0.0) and fo.total_key(0.0) < fo.total_key(5e-324)
    free = [F(b) for b in fo.NAN_FREE]
    assert sorted(free, key=fo.total_key) == sorted(free, key=lambda x: (x, math.copysign(1.0, x)))      # wide_group_ref._order where no NaN goes in
    assert len({fo.total_key(x) for x in POOL}) == 20


def _column(seed, n, with_nan=True, null_every=7):
    r = np.random.default_rng(seed)
    pool = POOL if with_nan else POOL[4:]
    return [None if null_every and k % null_every == 3 else pool[int(x)] for k, x in enumerate(r.integers(0, len(pool), n))]


def test_key_against_numpy_and_pyarrow():
    for seed in range(3):
        col = [v for v in _column(seed, 400) if v is not None]
        mine = sorted(range(len(col)), key=lambda i: fo.key(col[i]))
        # numpy's stable argsort puts NaNs last and ties the zeros: compare by the rule's classes (which NaN stands where among the NaNs is numpy's
        # business only in that it is stable -- and it is: the index sequences agree)
        assert mine == np.argsort(np.array([fo.bits(v) for v in col], dtype=np.uint64).view(np.float64), kind="stable").tolist()
        # pyarrow ascending, NULLs last: numbers, then NaNs, then NULLs, every tie in input order
        col = _column(seed, 400)
        idx = [i for i in range(len(col)) if col[i] is not None]
        mine = sorted(idx, key=lambda i: fo.key(col[i])) + [i for i in range(len(col)) if col[i] is None]
        arr = f64_array(col)
        assert pac.sort_indices(pa.table({"x": arr}), sort_keys=[("x", "ascending")]).to_pylist() == mine
        # as the first and as the second key of a two-key sort
        small = pa.array([k % 3 for k in range(len(col))], pa.int32())
        tbl = pa.table({"x": arr, "k": small, "id": pa.array(range(len(col)), pa.int64())})
        second = sorted(mine, key=lambda i: i % 3)                          # (stable: within a k, the order of `mine`)
        assert pac.sort_indices(tbl, sort_keys=[("k", "ascending"), ("x", "ascending"), ("id", "ascending")]).to_pylist() == second
        first = sorted(sorted(range(len(col)), key=lambda i: -(i % 3)), key=lambda i: (1, 0) if col[i] is None else (0, fo.key(col[i])))
        assert pac.sort_indices(tbl, sort_keys=[("x", "ascending"), ("k", "descending"), ("id", "ascending")]).to_pylist() == first
        # descending: on NaN-free columns only
        col = _column(seed, 400, with_nan=False)
        idx = [i for i in range(len(col)) if col[i] is not None]
        mine = sorted(idx, key=lambda i: fo.key(col[i]), reverse=True) + [i for i in range(len(col)) if col[i] is None]
        tbl = pa.table({"x": f64_array(col)})
        assert pac.sort_indices(tbl, sort_keys=[("x", "descending")]).to_pylist() == mine


def test_the_issue_s_column_sorts_as_stated():
    """0xFFF8..., 0x7FF8...01, both zeros, +-inf, +-5e-324 and a NULL: numbers, then both NaNs in input order, then the NULL"""
    col = [F(0xFFF8000000000000), 0.0, math.inf, F(0x7FF8000000000001), -5e-324, None, -0.0, -math.inf, 5e-324]
    mine = sorted([i for i in range(9) if col[i] is not None], key=lambda i: fo.key(col[i])) + [5]
    assert mine == [7, 4, 1, 6, 8, 2, 0, 3, 5]
    assert pac.sort_indices(pa.table({"x": f64_array(col)}), sort_keys=[("x", "ascending")]).to_pylist() == mine


def test_every_pattern_survives_the_round_trip_bit_for_bit():
    """table -> array -> record batch -> Python, from the buffer and from a Python list (what tests/test_plan_differential.py's _batches does)"""
    vals = POOL + [None] + POOL[::-1]
    t = {"f": vals, "id": list(range(len(vals)))}
    rb = batch([("f", "Float64"), ("id", "Int64")], t, slots={"f": {20: 0xFFF8000000000001}})
    assert [None if v is None else fo.bits(v) for v in rb.column(0).to_pylist()] == [None if v is None else fo.bits(v) for v in vals]
    assert np.frombuffer(rb.column(0).buffers()[1], dtype=np.uint64).tolist()[20] == 0xFFF8000000000001          # the NULL's slot holds what was put there
    listed = pa.record_batch([pa.array(vals, pa.float64())], names=["f"])
    assert [None if v is None else fo.bits(v) for v in listed.column(0).to_pylist()] == [None if v is None else fo.bits(v) for v in vals]
    u = np.array(fo.SPECIALS, dtype=np.uint64)
    assert np.array_equal(np.frombuffer(pa.array(u.view(np.float64)).buffers()[1], dtype=np.uint64), u)
    assert [r[0][1] % 2**64 for r in _norm([(v,) for v in POOL])] == fo.SPECIALS                     # what the comparisons below compare


# the casts of section "Casts": (target, value, what TRY_CAST gives -- None: does not fit)
NNAN = F(0xFFF8000000000000)
CASTS = [("Int32", 2147483647.0, 2147483647), ("Int32", 2147483647.9, 2147483647), ("Int32", 2147483648.0, None), ("Int32", -2147483648.0, -2147483648),
         ("Int32", -2147483648.9, -2147483648), ("Int32", -2147483649.0, None),
         ("Int64", 9223372036854774784.0, 9223372036854774784), ("Int64", 9223372036854775808.0, None), ("Int64", -9223372036854775808.0, -2**63),
         ("Int64", -9223372036854777856.0, None),
         ("UInt64", -0.0, 0), ("UInt64", -0.9, 0), ("UInt64", -1.0, None), ("UInt64", 18446744073709549568.0, 18446744073709549568), ("UInt64", 18446744073709551616.0, None)]
CASTS += [(ty, v, None) for ty in ("Int32", "Int64", "UInt64") for v in (math.nan, NNAN, math.inf, -math.inf)] + [(ty, 5e-324, 0) for ty in ("Int32", "Int64", "UInt64")]
# integer -> Float64: (source type, value, the double it rounds to)
ROUNDS = [("Int64", 2**53 + 1, 2.0**53), ("Int64", 2**53 + 3, 2.0**53 + 4), ("Int64", 2**63 - 1, 2.0**63), ("UInt64", 2**64 - 1, 2.0**64),
          ("UInt64", 2**63 + 1025, 2.0**63 + 2048), ("Int64", -(2**53 + 1), -(2.0**53))]


def test_the_typed_evaluator_casts_as_the_hand_written_list_says():
    assert -9223372036854777856.0 == np.nextafter(-2.0**63, -np.inf) and 9223372036854774784.0 == np.nextafter(2.0**63, 0.0)
    assert 18446744073709549568.0 == np.nextafter(2.0**64, 0.0)
    for ty, v, out in CASTS:
        assert g._cast(v, ty, True) == out and type(g._cast(v, ty, True)) in (int, type(None)), (ty, v)
        if out is None:
            with pytest.raises(g.ExprError):
                g._cast(v, ty, False)
        else:
            assert g._cast(v, ty, False) == out
        # pyarrow's checked cast of the truncated value, where it can say: it fits exactly when ours does
        if not math.isnan(v):
            try:
                got = pac.cast(pa.array([float(np.trunc(v))], pa.float64()), _PA[ty]).to_pylist()[0]
            except pa.ArrowInvalid:
                got = None
            assert got == out, (ty, v, got)
    for ty, v, out in ROUNDS:
        assert g._cast(v, "Float64", False) == out and fo.bits(g._cast(v, "Float64", False)) == fo.bits(out), (ty, v)
        assert pac.cast(pa.array([v], _PA[ty]), pa.float64(), safe=False).to_pylist()[0] == out


# ------------------------------------------------------------------ sort
SORT_COLS = [("f", "Float64"), ("id", "Int64")]


def _sort_node(desc, nulls_first):
    return pc.sort(pc.scan(SORT_COLS), [("f", desc, nulls_first)])          # NO tiebreak key: the row sequence carries the stability claim


def _by_rule(vals, desc, nulls_first):
    """the A-FO1 order of the rows, from float_order_ref alone"""
    live = sorted([i for i, v in enumerate(vals) if v is not None], key=lambda i: fo.key(vals[i]), reverse=desc)
    nulls = [i for i, v in enumerate(vals) if v is None]
    return nulls + live if nulls_first else live + nulls


def _check_sort(gpu, vals, desc, nulls_first, cuts=None, slots=None):
    t = {"f": vals, "id": list(range(len(vals)))}
    node = _sort_node(desc, nulls_first)
    order = _by_rule(vals, desc, nulls_first)
    expected = _norm([(vals[i], i) for i in order])
    assert want(node, t) == expected                                         # the interpreter follows the rule
    got = run(gpu, node, SORT_COLS, t, cuts, slots, must_run=("sort_norm_kernel",))
    if got != expected:
        diff = [(k, a, b) for k, (a, b) in enumerate(zip(got, expected)) if a != b][:4]
        pytest.fail("%d rows; first differing (position, got, expected): %r" % (len(got), diff))


def _pool_column():
    """every pattern three times, equal-by-rule values far apart (a stride of 7 over 20 patterns), a NULL every 9 rows whose slot holds a NaN"""
    vals, slots = [], {}
    for k in range(60):
        if k % 9 == 4:
            slots[len(vals)] = 0xFFF8000000000000 + k
            vals.append(None)
        vals.append(POOL[(k * 7) % 20])
    return vals, {"f": slots}


@pytest.mark.gpu
@pytest.mark.parametrize("desc,nulls_first", OPTIONS)
def test_sort_of_the_pool(gpu, desc, nulls_first):
    vals, slots = _pool_column()
    assert sum(v is None for v in vals) == 7 and len(vals) == 67 and all(sum(fo.bits(v) == b for v in vals if v is not None) == 3 for b in fo.SPECIALS)
    _check_sort(gpu, vals, desc, nulls_first, slots=slots)


def _seam_column(n):
    """n rows, no negative number: 12 zeros of mixed sign, 12 NaNs of the four patterns, 5 NULLs, distinct positive numbers, spread over the input
    by a fixed permutation.  Ascending (NULLs first) the NaNs are the last 12 rows, descending (NULLs first) the zeros are."""
    vals = [0.0, -0.0, -0.0, 0.0] * 3 + POOL[:4] * 3 + [None] * 5 + [k / 4 for k in range(1, n - 28)]
    perm = np.random.default_rng(11).permutation(n)
    return [vals[int(p)] for p in perm]


@pytest.mark.gpu
@pytest.mark.parametrize("desc,nulls_first", OPTIONS)
def test_sort_across_the_tile_seam(gpu, desc, nulls_first):
    vals = _seam_column(4097)
    if nulls_first:                                                          # a run of ties of mixed patterns lies across output rows 4095 | 4096
        tail = [vals[i] for i in _by_rule(vals, desc, True)[4090:]]
        assert len({fo.key(v) for v in tail}) == 1 and len({fo.bits(v) for v in tail}) > 1 and math.isnan(tail[0]) == (not desc)
    _check_sort(gpu, vals, desc, nulls_first)


@pytest.mark.gpu
@pytest.mark.parametrize("desc,nulls_first", [(False, False), (True, True)])
def test_sort_over_batches(gpu, desc, nulls_first):
    _check_sort(gpu, _seam_column(4200), desc, nulls_first, cuts=[0, 1, 4095, 4097, 4200])


@pytest.mark.gpu
@pytest.mark.parametrize("desc", [False, True])
def test_a_constant_sub_key_is_the_identity(gpu, desc):
    """every row ties: only NaNs (four patterns), only zeros (both signs)"""
    for vals in ([POOL[(k * 3) % 4] for k in range(300)], [0.0 if (k * k) % 3 else -0.0 for k in range(300)]):
        assert _by_rule(vals, desc, False) == list(range(300)) and len({fo.bits(v) for v in vals}) > 1
        _check_sort(gpu, vals, desc, False)


# ------------------------------------------------------------------ window
WIN_COLS = [("p", "Int32"), ("f", "Float64"), ("v", "Int64"), ("m", "Float64"), ("id", "Int64")]


def _window_node(part):
    a = pc.scan(WIN_COLS)
    node = pc.window(a, [("count", None, part, ["f"]), ("sum", "v", part, ["f"]), ("max", "m", part, ["f"]), ("row_number", None, ["f"], [])])
    return pc.keep(node, [n for n, _ in node.cols[:4]] + ["id"])


@pytest.mark.gpu
def test_window_peer_groups_by_hand(gpu):
    """the rows arrive sorted by f (A-FO1): -1.0, three zeros, three NaNs, two NULLs.  RANGE ... CURRENT ROW: every peer receives its group's end"""
    nan, nnan, snan = POOL[0], POOL[1], POOL[2]
    t = {"p": [1] * 9, "f": [-1.0, 0.0, -0.0, 0.0, nan, nnan, snan, None, None], "v": list(range(1, 10)),
         "m": [5.0, -0.0, 0.0, -math.inf, 5e-324, 7.0, None, 1.0, 9.0], "id": list(range(9))}
    node = _window_node([])
    count = [1, 4, 4, 4, 7, 7, 7, 9, 9]
    total = [1, 10, 10, 10, 28, 28, 28, 45, 45]
    high = [5.0, 5.0, 5.0, 5.0, 7.0, 7.0, 7.0, 9.0, 9.0]
    rn = [1, 1, 2, 3, 1, 2, 3, 1, 2]
    expected = _norm(list(zip(count, total, high, rn, range(9))))
    assert want(node, t) == expected
    assert run(gpu, node, WIN_COLS, t, slots={"f": {7: 0x7FF8000000000000, 8: 0xFFFFFFFFFFFFFFFF}}, must_run=("win_tile_kernel", "win_emit_kernel", "run_rank_kernel")) == expected


def _seamed_table():
    """4097 rows sorted by (p, f): in every partition negatives, the peer group {+0.0, -0.0, +0.0}, positives, a group of three NaN patterns.  The
    zero groups lie across rows 7 | 8 (a lane's eight rows), 511 | 512 (a wave) and 2047 | 2048 (a tile), the NaN groups across 15 | 16, 1023 | 1024
    and 4095 | 4096"""
    zeros, nans = [0.0, -0.0, 0.0], [POOL[1], POOL[2], POOL[0]]
    f, p = [], []
    for part, (z_at, nan_at) in enumerate([(6, 14), (510, 1022), (2046, 4094)]):
        start = len(f)
        f += [-(z_at - start - k) / 4 for k in range(z_at - start)] + zeros
        f += [(k + 1) / 4 for k in range(nan_at - len(f))] + nans
        p += [part] * (len(f) - start)
    assert len(f) == 4097 and all(f[k:k + 3] == zeros and [math.copysign(1, x) for x in f[k:k + 3]] == [1, -1, 1] for k in (6, 510, 2046))
    assert all(math.isnan(x) for k in (14, 1022, 4094) for x in f[k:k + 3])
    r = np.random.default_rng(4)
    m = [None if k % 13 == 5 else POOL[4:][int(x)] for k, x in enumerate(r.integers(0, 16, 4097))]
    return {"p": p, "f": f, "v": [int(x) for x in r.integers(-1000, 1000, 4097)], "m": m, "id": list(range(4097))}


@pytest.mark.gpu
def test_window_peer_groups_across_lane_wave_and_tile(gpu):
    t = _seamed_table()
    node = _window_node(["p"])
    expected = want(node, t)
    assert [expected[k][0] for k in (6, 7, 8)] == [9, 9, 9] and [expected[k][0] for k in (14, 15, 16)] == [17, 17, 17]      # COUNT through the group's end
    assert [expected[k][3] for k in (2046, 2047, 2048)] == [1, 2, 3] and [expected[k][3] for k in (4094, 4095, 4096)] == [1, 2, 3]
    got = run(gpu, node, WIN_COLS, t, must_run=("win_tile_kernel", "win_carry_kernel", "win_emit_kernel", "run_rank_kernel"))
    if got != expected:
        pytest.fail("first differing (row, got, expected): %r" % [(k, a, b) for k, (a, b) in enumerate(zip(got, expected)) if a != b][:4])


@pytest.mark.gpu
def test_a_null_key_between_two_zeros_is_its_own_group(gpu):
    """the slot of the NULL holds a NaN pattern (and, in the second table, a zero): it is never compared"""
    for slot in (0xFFF8000000000000, 0x8000000000000000):
        t = {"p": [1, 1, 1], "f": [0.0, None, -0.0], "v": [1, 2, 4], "m": [1.0, 2.0, 3.0], "id": [0, 1, 2]}
        node = _window_node([])
        expected = _norm([(1, 1, 1.0, 1, 0), (2, 3, 2.0, 1, 1), (3, 7, 3.0, 1, 2)])
        assert want(node, t) == expected
        assert run(gpu, node, WIN_COLS, t, slots={"f": {1: slot}}) == expected


# ------------------------------------------------------------------ filters
PAIR_COLS = [("x", "Float64"), ("y", "Float64"), ("id", "Int64")]


def _pairs():
    xs, ys = zip(*itertools.product(POOL, POOL))
    return {"x": list(xs), "y": list(ys), "id": list(range(len(xs)))}


def _ids(rows):
    return [r[-1] for r in rows]


@pytest.mark.gpu
@pytest.mark.parametrize("op", sorted(NP_CMP))
def test_truth_table_of_column_pairs(gpu, op):
    """every pattern of the pool against every pattern (20 x 20: the whole pool, NaNs included), on the one-pass leaf and on the general evaluator (a
    computed right side, and the comparison as a projected flag), against numpy's IEEE comparison of the same bits"""
    t = _pairs()
    x, y = (np.array([fo.bits(v) for v in t[c]], dtype=np.uint64).view(np.float64) for c in "xy")
    truth = NP_CMP[op](x, y)
    assert 0 < truth.sum() < len(truth)
    a = pc.scan(PAIR_COLS)
    fused = pc.keep(pc.filt(a, pc.binop(a.c("x"), op, a.c("y"))), ["id"])
    assert _ids(run(gpu, fused, PAIR_COLS, t, must_run=("pred_flag_kernel",))) == np.flatnonzero(truth).tolist()
    general = pc.keep(pc.filt(a, pc.binop(a.c("x"), op, pc.binop(a.c("y"), "Plus", pc.lit("Float64", 0.0)))), ["id"])
    assert _ids(run(gpu, general, PAIR_COLS, t, must_run=("valprog_kernel",))) == np.flatnonzero(truth).tolist()
    flag = pc.proj(a, [(pc._flag(pc.binop(a.c("x"), op, a.c("y"))), "is", "Int32"), (a.c("id"), "id", "Int64")])
    assert [r[0] for r in run(gpu, flag, PAIR_COLS, t, must_run=("valprog_kernel",))] == truth.astype(int).tolist()


LITERALS = pc.FLOAT_LITERALS + [-1.7976931348623157e308, 2.2250738585072014e-308]


@pytest.mark.gpu
@pytest.mark.parametrize("op", sorted(NP_CMP))
def test_column_against_literals_under_kleene_logic(gpu, op):
    """x and y hold the pool and NULLs (every pair of {pattern, NULL}); `x op L` alone, with the literal on the left, and under AND / OR / NOT with a
    second nullable comparison, so that every row of the Kleene tables meets a NaN: against numpy for the single leaf, the interpreter for the rest"""
    vals = POOL + [None]
    xs, ys = zip(*itertools.product(vals, vals))
    t = {"x": list(xs), "y": list(ys), "id": list(range(len(xs)))}
    live = np.array([v is not None for v in xs])
    x = np.array([0 if v is None else fo.bits(v) for v in xs], dtype=np.uint64).view(np.float64)
    a = pc.scan(PAIR_COLS)
    for literal in LITERALS:
        lit = pc.lit("Float64", literal)
        one = pc.keep(pc.filt(a, pc.binop(a.c("x"), op, lit)), ["id"])
        truth = NP_CMP[op](x, np.float64(literal)) & live
        assert _ids(run(gpu, one, PAIR_COLS, t, must_run=("pred_flag_kernel",))) == _ids(want(one, t)) == np.flatnonzero(truth).tolist(), literal
        left = pc.keep(pc.filt(a, pc.binop(lit, op, a.c("x"))), ["id"])
        assert _ids(run(gpu, left, PAIR_COLS, t)) == np.flatnonzero(NP_CMP[op](np.float64(literal), x) & live).tolist(), literal
    lit = pc.lit("Float64", 0.0)
    second = pc.binop(a.c("y"), "LtEq", pc.lit("Float64", 5e-324))
    for pred in (pc.binop(pc.binop(a.c("x"), op, lit), "And", second), pc.binop(pc.binop(a.c("x"), op, lit), "Or", second),
                 pc._not(pc.binop(pc.binop(a.c("x"), op, lit), "Or", pc._not(second))),
                 pc.binop({"physical_expr": "is_null_expr", "arg": a.c("y")}, "Or", pc._not(pc.binop(a.c("x"), op, a.c("y"))))):
        node = pc.keep(pc.filt(a, pred), ["id"])
        assert run(gpu, node, PAIR_COLS, t, must_run=("pred_flag_kernel",)) == want(node, t)
        flags = pc.proj(a, [(pc._flag(pred), "is", "Int32"), (a.c("id"), "id", "Int64")])          # TRUE / FALSE / NULL told apart, on the general evaluator
        assert run(gpu, flags, PAIR_COLS, t, must_run=("valprog_kernel",)) == want(flags, t)


INT_COLS = [("x", "Int32"), ("id", "Int64")]
INT_VALUES = [-2**31, -2**31 + 1, -1, 0, 1, 2**31 - 2, 2**31 - 1, None]
INT_LITERALS = [-2147483648.5, -2147483648.0, -2147483647.5, -0.5, -0.0, 0.5, 2147483646.5, 2147483647.0, 2147483647.5, 2147483648.0, 1e300, -1e300]


@pytest.mark.gpu
@pytest.mark.parametrize("op", sorted(PY_CMP))
def test_int32_column_against_float64_literals(gpu, op):
    """the planner turns `x op f` into an integer comparison (x < f <=> x < ceil f, ...): against Python's float(x) op f, which is exact -- every
    Int32 is a double"""
    t = {"x": INT_VALUES * 3, "id": list(range(24))}
    a = pc.scan(INT_COLS)
    for literal in INT_LITERALS:
        node = pc.keep(pc.filt(a, pc.binop(a.c("x"), op, pc.lit("Float64", literal))), ["id"])
        expected = [k for k, v in enumerate(t["x"]) if v is not None and PY_CMP[op](float(v), literal)]
        assert _ids(run(gpu, node, INT_COLS, t)) == expected, literal


# ------------------------------------------------------------------ casts
CAST_COLS = [("f", "Float64"), ("l", "Int64"), ("u", "UInt64"), ("id", "Int64")]


def _cast_table(values):
    n = len(values)
    return {"f": list(values), "l": [0] * n, "u": [0] * n, "id": list(range(n))}


@pytest.mark.gpu
def test_try_cast_gives_null_where_the_value_does_not_fit(gpu):
    values = sorted({v for _, v, _ in CASTS if not math.isnan(v)}) + [math.nan, NNAN, None]
    t = _cast_table(values)
    a = pc.scan(CAST_COLS)
    node = pc.proj(a, [(pc.cast(a.c("f"), ty, safe=True), "to_" + ty, ty) for ty in ("Int32", "Int64", "UInt64")] + [(a.c("id"), "id", "Int64")])
    expected = [tuple(None if v is None else g._cast(v, ty, True) for ty in ("Int32", "Int64", "UInt64")) + (k,) for k, v in enumerate(values)]
    for ty, v, out in CASTS:                                                 # the hand-written list is in it
        k = next(k for k, w in enumerate(values) if w is not None and fo.bits(w) == fo.bits(v))
        assert expected[k][("Int32", "Int64", "UInt64").index(ty)] == out, (ty, v)
    assert want(node, t) == expected
    assert run(gpu, node, CAST_COLS, t, must_run=("valprog_kernel",)) == expected


@pytest.mark.gpu
@pytest.mark.parametrize("ty,bad,good", [("Int32", 2147483648.0, 2147483647.9), ("Int64", 9223372036854775808.0, -9223372036854775808.0),
                                         ("UInt64", -1.0, -0.9)])
def test_cast_fails_the_call_where_the_value_does_not_fit(gpu, ty, bad, good):
    from flock_amd import FlockGpuError, _ffi
    a = pc.scan(CAST_COLS)
    node = pc.proj(a, [(pc.cast(a.c("f"), ty), "x", ty), (a.c("id"), "id", "Int64")])
    for worst in (bad, math.nan, NNAN, -math.inf):
        t = _cast_table([1.0, good, worst, None])
        with pytest.raises(g.ExprError):
            run_plan(node.plan, [t])
        with pytest.raises(FlockGpuError) as e:
            run(gpu, node, CAST_COLS, t)
        assert e.value.code == _ffi.ERR_INVALID and "a value does not fit the type it is cast to" in str(e.value), str(e.value)
    t = _cast_table([1.0, good, None])                                       # the context then runs a good plan
    assert run(gpu, node, CAST_COLS, t) == want(node, t) == [(1, 0), (g._cast(good, ty, False), 1), (None, 2)]


@pytest.mark.gpu
def test_integers_round_to_the_nearest_even_double(gpu):
    t = {"f": [0.0] * 8, "l": [v for ty, v, _ in ROUNDS if ty == "Int64"] + [None, 2**53, -2**63, 0], "u": [v for ty, v, _ in ROUNDS if ty == "UInt64"] + [None, 0, 2**53 + 1, 2**64 - 1025, 2**64 - 1024, 1],
         "id": list(range(8))}
    a = pc.scan(CAST_COLS)
    node = pc.proj(a, [(pc.cast(a.c("l"), "Float64"), "fl", "Float64"), (pc.cast(a.c("u"), "Float64"), "fu", "Float64"), (a.c("id"), "id", "Int64")])
    expected = _norm([(None if l is None else g._cast(l, "Float64", False), None if u is None else g._cast(u, "Float64", False), k)
                      for k, (l, u) in enumerate(zip(t["l"], t["u"]))])
    by_hand = {(ty, v): _norm([(out,)])[0][0] for ty, v, out in ROUNDS}
    for k, (l, u) in enumerate(zip(t["l"], t["u"])):
        assert expected[k][0] == by_hand.get(("Int64", l), expected[k][0]) and expected[k][1] == by_hand.get(("UInt64", u), expected[k][1])
    assert sum(("Int64", l) in by_hand for l in t["l"]) + sum(("UInt64", u) in by_hand for u in t["u"]) == len(ROUNDS)
    assert want(node, t) == expected
    assert run(gpu, node, CAST_COLS, t, must_run=("valprog_kernel",)) == expected


# ------------------------------------------------------------------ refusals
def _float_key_plans():
    a, b = pc.scan([("f", "Float64"), ("k", "Int64"), ("v", "Int64")]), pc.scan([("g", "Float64"), ("w", "Int64")])
    return {"group_by": (pc.aggregate(a, ["f"], [("count", None)]), "execute", "GROUP BY a Float64 column"),
            "distinct": (pc.aggregate(pc.keep(a, ["f"]), ["f"], []), "execute", "GROUP BY a Float64 column"),
            "count_distinct": (pc.aggregate(a, ["k"], [("dc", "f")]), "explain", "distinct_count needs an integer or Utf8 column"),
            "inner_join": (pc.join("Inner", a, b, [("f", "g")]), "execute", "join keys must be integer columns of one signedness, or two Utf8 columns"),
            "semi_join": (pc.join("Semi", a, b, [("f", "g")]), "explain", "join keys must be integer columns of one signedness, or two Utf8 columns")}


@pytest.mark.parametrize("which", sorted(_float_key_plans()))
def test_float64_keys_are_refused_by_name_at_explain_where_explain_looks(which):
    """A-FO1 / A-FO2 say how doubles ORDER and TIE; nothing hashes them.  COUNT(DISTINCT) and the Semi / Anti join's key types are refused by
    flockgpu_plan_explain; GROUP BY, DISTINCT and the Inner join's keys pass explain (it does not look at key types there) and are refused by
    the execute: test_float64_keys_are_refused_by_name_at_execute"""
    from flock_amd import FlockGpuError, _ffi
    from flock_amd.runtime import explain
    node, where, message = _float_key_plans()[which]
    if where == "execute":
        assert "Float64" in explain(node.plan)
        return
    with pytest.raises(FlockGpuError) as e:
        explain(node.plan)
    assert e.value.code == _ffi.ERR_UNSUPPORTED and message in str(e.value), str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(k for k, v in _float_key_plans().items() if v[1] == "execute"))
def test_float64_keys_are_refused_by_name_at_execute(gpu, which):
    from flock_amd import FlockGpuError, _ffi
    node, _, message = _float_key_plans()[which]
    left = {"f": [0.0, -0.0, math.nan, 1.0], "k": [1, 2, 3, 4], "v": [1, 1, 1, 1]}
    feeds = [[batch([("f", "Float64"), ("k", "Int64"), ("v", "Int64")], left)]]
    if which == "inner_join":
        feeds.append([batch([("g", "Float64"), ("w", "Int64")], {"g": [0.0, math.nan], "w": [1, 2]})])
    with pytest.raises(FlockGpuError) as e:
        _execute(gpu, node.plan, feeds, True)
    assert e.value.code == _ffi.ERR_UNSUPPORTED and message in str(e.value), str(e.value)
