"""Plan ingest (flock_amd/csrc/plan_feed.hip): what a refused feed leaves behind on each of the three entry points, and a prefetched pane
with a Utf8 column, whose raw end offsets are rebased run by run when the pane is appended."""
import numpy as np
import pyarrow as pa
import pytest

import oracle
from oracle import generic_ops as g
from test_plan_boundary import _auction_batches, _person_batches, _plan
from test_plan_round4 import _agg_plan, _null_batches, _null_table, _pyrows


@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


_AGGS = [("count", "v", "UInt64"), ("max", "v", "Int64"), ("count", None, "UInt64")]


def _agg_want(tables):
    window = {c: [x for t in tables for x in t[c]] for c in ("k", "v", "f", "s")}
    want = g.hash_aggregate_exec(window, ["k"], [("%s(%s)" % (fn.upper(), col or "UInt8(1)"), fn, col) for fn, col, _ in _AGGS])
    return sorted(g.rows(want), key=lambda r: (r[0] is None, r[0] or 0))


def _agg_got(rb):
    return sorted(_pyrows(rb), key=lambda r: (r[0] is None, r[0] or 0))


@pytest.mark.gpu
def test_refused_feeds_leave_leaf_and_ring_as_they_were(gpu):
    """A batch that lacks a column the plan reads (INVALID) and one whose Int32 key arrives as Int64 (UNSUPPORTED), handed to feed without a
    ring, to feed_pane on an open ring behind one good pane, and to prefetch_pane on that ring: each is refused with its code, the ring's
    state stays what it was, and the good batches fed afterwards give exactly the oracle's groups over the good rows."""
    from flock_amd import FlockGpuError, _ffi
    from flock_amd.runtime import ExecutionContext, collect
    good = [_null_table(300, 21), _null_table(260, 22)]
    r = np.random.default_rng(23)
    k, v = r.integers(-3, 6, 200), r.integers(-50, 50, 200)        # (no NULLs: a prefetch refuses those before it looks further)
    f, s = pa.array(np.round(r.normal(0, 10, 200))), pa.array(["s1"] * 200)
    bad = [(pa.record_batch([pa.array(k, pa.int32()), f, s], names=["k", "f", "s"]), _ffi.ERR_INVALID),
           (pa.record_batch([pa.array(k, pa.int64()), pa.array(v, pa.int64()), f, s], names=["k", "v", "f", "s"]), _ffi.ERR_UNSUPPORTED)]

    def refused(call, code):
        with pytest.raises(FlockGpuError) as e:
            call()
        assert e.value.code == code

    ctx = ExecutionContext([_agg_plan(_AGGS)], name="ingest-plain", gpu=gpu)
    plan = ctx.plans[0]
    plan.feed(0, _null_batches(good[0], 110))
    for rb, code in bad:
        refused(lambda: plan.feed(0, [rb]), code)
    plan.feed(0, _null_batches(good[1], 90))
    assert _agg_got(ctx.execute()[0][0]) == _agg_want(good)
    ctx.clean_data_sources()

    ctx.open_window_ring(2)
    assert _agg_got(collect(ctx, [[_null_batches(good[0], 110)]], pane=0)[0][0]) == _agg_want(good[:1])
    state = plan.ring_state()
    for rb, code in bad:
        refused(lambda: plan.feed(0, [rb], pane=1), code)
        assert plan.ring_state() == state
        if code == _ffi.ERR_UNSUPPORTED:   # (the one code `prefetch` answers with False: the pane is to be fed the ordinary way)
            assert plan.prefetch(0, [rb], 1) is False
        else:
            refused(lambda: plan.prefetch(0, [rb], 1), code)
        assert plan.ring_state() == state
    assert _agg_got(collect(ctx, [[_null_batches(good[1], 90)]], pane=1)[0][0]) == _agg_want(good)
    assert plan.ring_state() == (1, 1, 2)
    ctx.close()


def _blank_text(rb):
    """`rb` with every Utf8 value replaced by the empty string."""
    return pa.record_batch([pa.array([""] * rb.num_rows, pa.string()) if pa.types.is_string(c.type) else c for c in rb.columns], names=rb.schema.names)


def _q8_want(persons, auctions):
    """NEXMark q8 over the fed batches themselves: (p_id, name) of the persons who sell in the window."""
    ids = [x for rb in persons for x in rb["p_id"].to_pylist()]
    names = [x for rb in persons for x in rb["name"].to_pylist()]
    raw = [x.encode() for x in names]
    off = np.zeros(len(raw) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in raw])
    data = np.frombuffer(b"".join(raw) + b"\0", np.uint8).copy()
    sellers = np.array([x for rb in auctions for x in rb["seller"].to_pylist()], np.int32)
    rows = oracle.q8_join(np.array(ids, np.int32), oracle.Utf8(off, data), sellers)
    return sorted((ids[i], names[i]) for i in rows)


@pytest.mark.gpu
def test_prefetched_utf8_panes_equal_fed_panes(gpu):
    """q8 over Hopping(2 panes) with the person relation (a Utf8 column) prefetched and the auctions fed the ordinary way.  A pane's batches:
    two zero-copy slices of one table (they continue each other: one run, one rebase), a batch allocated on its own (a new run, a new
    delta), a batch whose strings are all empty; pane 2 holds no person at all.  Every window equals the ring fed the ordinary way and the
    oracle."""
    from flock_amd.runtime import ExecutionContext, collect
    eps, n_panes, ppw = 6_000, 5, 2
    s = oracle.NexmarkStream(seed=31, eps=eps)
    pers, aucs = [], []
    for p in range(n_panes):
        a, b, c, d = p * eps, p * eps + 3_100, p * eps + 4_700, (p + 1) * eps
        one = _person_batches(s, a, b, b - a)[0]
        cut = one.num_rows // 3 + 1
        pers.append([one.slice(0, cut), one.slice(cut), _person_batches(s, b, c, c - b)[0], _blank_text(_person_batches(s, c, d, d - c)[0])])
        aucs.append(_auction_batches(s, a, d, 2_500))
    pers[2] = [pers[2][2].slice(0, 0)]
    plain = ExecutionContext([_plan(8)], name="q8-plain", gpu=gpu)
    ahead = ExecutionContext([_plan(8)], name="q8-ahead", gpu=gpu)
    plain.open_window_ring(ppw)
    ahead.open_window_ring(ppw)
    plan = ahead.plans[0]
    ip = next(i for i in range(len(plan.inputs)) if plan.matches(i, pers[0][0].schema))
    ia = next(i for i in range(len(plan.inputs)) if plan.matches(i, aucs[0][0].schema))
    assert ip != ia and plan.prefetch(ip, pers[0], 0)
    total = 0
    for p in range(n_panes):
        plan.feed_prefetched(ip, p)
        plan.feed(ia, aucs[p], pane=p)
        if p + 1 < n_panes:
            assert plan.prefetch(ip, pers[p + 1], p + 1)               # ... on its way while window p executes
        got = ahead.execute()[0][0]
        ahead.clean_data_sources()
        ref = collect(plain, [[pers[p]], [aucs[p]]], pane=p)[0][0]
        lo = max(0, p - ppw + 1)
        want = _q8_want([rb for q in range(lo, p + 1) for rb in pers[q]], [rb for q in range(lo, p + 1) for rb in aucs[q]])
        rows = lambda rb: sorted(zip(rb["p_id"].to_pylist(), rb["name"].to_pylist()))
        assert rows(got) == rows(ref) == want, p
        total += len(want)
    assert total > 20 and any(name == "" for _, name in want)
    plain.close()
    ahead.close()
