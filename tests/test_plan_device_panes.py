"""Panes of the device-side window ring fed from device columns (flockgpu_plan_feed_pane_columns) against the same panes fed from the host
(flockgpu_plan_feed_pane): q5's state ring and the rows ring, Utf8 columns and NULLs, host and device panes in one ring, the refusals, and text in ->
event-time panes (flockgpu_pane_split) -> ring -> text out."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

import device_feed_util as dfu
import oracle
from device_feed_util import FLAG_TILE
from test_plan_boundary import TS, _plan

pytestmark = pytest.mark.gpu
BID = [("auction", "int32"), ("bidder", "int32"), ("price", "int32"), ("b_date_time", "timestamp_ms")]


@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    ctx = GpuContext(0)
    yield ctx
    ctx.close()


def _q5_rows(rb):
    return sorted(zip(rb["auction"].to_pylist(), rb["num"].to_pylist()))


def bid_batch(b, lo, hi):
    return pa.record_batch([pa.array(b["auction"][lo:hi]), pa.array(b["bidder"][lo:hi]), pa.array(b["price"][lo:hi]), pa.array(b["b_date_time"][lo:hi]).cast(TS)],
                           names=[n for n, _ in BID])


def bid_source(b, lo, hi):
    import torch
    return [(n, t, torch.from_numpy(np.ascontiguousarray(b[n][lo:hi])).to("cuda:0")) for n, t in BID], {}


@pytest.fixture(scope="module")
def q5_panes():
    """8 panes of 8 000 to 16 000 bids -- but one is empty, one holds 1 row and one FLAG_TILE + 1 rows -- as host batches and device sources"""
    sizes = [9_000, 12_000, 0, 1, FLAG_TILE + 1, 16_000, 8_000, 10_000]
    b = oracle.NexmarkStream(seed=41, eps=10_000).bids(0, 80_000)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    assert cuts[-1] <= len(b["auction"])
    host = [[bid_batch(b, int(cuts[p]), int(cuts[p + 1]))] if sizes[p] else [] for p in range(len(sizes))]
    device = [bid_source(b, int(cuts[p]), int(cuts[p + 1])) for p in range(len(sizes))]
    return host, device


@pytest.mark.parametrize("generic_only", [False, True])
@pytest.mark.parametrize("ppw", [2, 3])
def test_q5_device_panes_equal_host_panes_equal_whole_windows(gpu, q5_panes, generic_only, ppw):
    from flock_amd.runtime import ExecutionContext, collect, collect_device
    host, device = q5_panes
    ring_d = ExecutionContext([_plan(5)], name="q5-dev", gpu=gpu, generic_only=generic_only)
    ring_h = ExecutionContext([_plan(5)], name="q5-host", gpu=gpu, generic_only=generic_only)
    whole = ExecutionContext([_plan(5)], name="q5-whole", gpu=gpu, generic_only=generic_only)
    ring_d.open_window_ring(ppw)
    ring_h.open_window_ring(ppw)
    for p in range(len(host)):
        got = collect_device(ring_d, [device[p]] if host[p] else [], pane=p)[0][0]
        want = collect(ring_h, [[host[p]]], pane=p)[0][0]
        ref = collect(whole, [[[b for q in range(max(0, p - ppw + 1), p + 1) for b in host[q]]]])[0][0]
        assert _q5_rows(got) == _q5_rows(want) == _q5_rows(ref), p
        assert got.schema == want.schema
        assert ring_d.plans[0].ring_state() == ring_h.plans[0].ring_state() == (max(0, p - ppw + 2), min(p + 1, ppw - 1), ppw)
    for ctx in (ring_d, ring_h, whole):
        ctx.close()


# ------------------------------------------------------------------ the rows ring: Utf8 columns and NULLs
def pane_table(n_panes=6, rows=700, seed=3, big=2):
    """a table and the row ranges of its panes; panes 0 and 1 hold no NULL at all (a NULL first appears in pane 2: the ring back-fills the validity of
    the panes before), pane `big` holds more than a flag tile of rows"""
    sizes = [rows + 37 * p for p in range(n_panes)]
    sizes[big] = FLAG_TILE + 3
    cuts = [0]
    for s in sizes:
        cuts.append(cuts[-1] + s)
    t = dfu.table("a", cuts[-1], seed)
    for name, vals in t.items():
        fill = next(v for v in vals if v is not None)
        for i in range(cuts[2]):
            if vals[i] is None:
                vals[i] = fill
    return t, [(cuts[p], cuts[p + 1]) for p in range(n_panes)]


def run_panes(gpu, plan, t, ranges, feeds, ppw=3, ordered=False, **dev_kw):
    """the windows of plan over the panes of t; feeds[p]: "host" | "device" | "both" (the pane's first half from the host, its second from the device)"""
    run = dfu.Run(gpu, plan)
    run.ctx.open_window_ring(ppw)
    out = []
    for p, (lo, hi) in enumerate(ranges):
        parts = {"host": [("host", lo, hi)], "device": [("device", lo, hi)], "both": [("host", lo, (lo + hi) // 2), ("device", (lo + hi) // 2, hi)],
                 "both2": [("device", lo, (lo + hi) // 2), ("host", (lo + hi) // 2, hi)]}[feeds[p]]
        for how, a, b in parts:
            if how == "host":
                run.p.feed(run.leaf[0], [dfu.host_batch(run.fields[0], t, a, b)], pane=p)
            else:
                columns, valid = dfu.device_source(run.fields[0], t, a, b, **dev_kw)
                run.p.feed_columns(run.leaf[0], columns, valid, pane=p)
        out.append((run.rows(ordered), run.p.ring_state()))
        run.ctx.clean_data_sources()
    run.close()
    return out


@pytest.mark.parametrize("kind", ["filter_project", "group_by"])
@pytest.mark.parametrize("validity,shift", [("nulls", 0), ("always", 0), ("nulls", 3), ("always", 3)])
def test_rows_ring_with_utf8_and_nulls_device_panes_equal_host_panes(gpu, kind, validity, shift):
    plan, _, _ = dfu.plan_of(kind)
    t, ranges = pane_table()
    if kind == "filter_project":                       # a pane of which the census drops every row: the filter's column is NULL all over it
        lo, hi = ranges[4]
        t["a_g"][lo:hi] = [None] * (hi - lo)
    # filter + projection keeps the rows' order: compared in order; the groups of a GROUP BY come in the order their hash table yields
    ordered = kind == "filter_project"
    want = run_panes(gpu, plan, t, ranges, ["host"] * len(ranges), ordered=ordered)
    got = run_panes(gpu, plan, t, ranges, ["device"] * len(ranges), ordered=ordered, validity=validity, shift=shift)
    assert len(want[-1][0]) > 0 and any(None in r for w in want for r in w[0])
    for p, (g, w) in enumerate(zip(got, want)):
        assert g[1] == w[1], p
        assert g[0] == w[0], p


def test_host_and_device_panes_alternate_in_one_ring_and_inside_one_pane(gpu):
    plan, _, _ = dfu.plan_of("filter_project")
    t, ranges = pane_table(seed=4)
    want = run_panes(gpu, plan, t, ranges, ["host"] * 6, ordered=True)
    for feeds in (["host", "device", "host", "device", "host", "device"], ["device", "both", "both2", "host", "both", "device"]):
        got = run_panes(gpu, plan, t, ranges, feeds, ordered=True, shift=3)
        assert got == want, feeds


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("generic_only", [False, True])
def test_order_errors_and_refused_columns_leave_the_ring_as_it_was(gpu, q5_panes, generic_only):
    import torch
    from flock_amd import FlockGpuError, _ffi
    from flock_amd.runtime import ExecutionContext
    host, device = q5_panes
    ctx = ExecutionContext([_plan(5)], gpu=gpu, generic_only=generic_only)
    plan = ctx.plans[0]

    def refused(code, fn, needle="pane"):
        with pytest.raises(FlockGpuError) as e:
            fn()
        assert e.value.code == code and needle in str(e.value), str(e.value)

    refused(_ffi.ERR_INVALID, lambda: plan.feed_columns(0, *device[0], pane=0), "ring")           # no ring open
    with pytest.raises(ValueError, match="ring"):
        ctx.feed_device_sources([device[0]], pane=0)
    ctx.open_window_ring(2)
    with pytest.raises(ValueError, match="ring"):
        ctx.feed_device_sources([device[0]])                                                     # a ring is open: panes only, as before
    with pytest.raises(ValueError):
        plan.feed_columns(0, *device[0], borrow=True, pane=4)
    ctx.feed_device_sources([device[0]], pane=4)
    ctx.feed_device_sources([device[1]], pane=5)
    want, state = _q5_rows(ctx.execute()[0][0]), plan.ring_state()
    assert state == (4, 2, 2)

    def unchanged():
        assert plan.ring_state() == state and _q5_rows(ctx.execute()[0][0]) == want

    for bad in (3, 4, 7, 6):                             # older than the ring, a closed pane, a skipped pane, the successor of a full ring
        refused(_ffi.ERR_INVALID, lambda: ctx.feed_device_sources([device[5]], pane=bad))
        unchanged()
    columns, valid = device[5]
    spec, rows, keep = gpu._text_columns(columns, valid)
    lib = _ffi.load()
    assert lib.flockgpu_plan_feed_pane_columns(plan.h, 0, 5, spec, len(columns), rows, _ffi.FEED_BORROW) == _ffi.ERR_INVALID
    assert "plan_feed_pane_columns:" in lib.flockgpu_last_error(gpu._h).decode()
    assert lib.flockgpu_plan_feed_pane_columns(plan.h, 0, 5, spec, len(columns), rows, 2) == _ffi.ERR_INVALID
    unchanged()
    refused(_ffi.ERR_INVALID, lambda: plan.feed_columns(0, [c for c in columns if c[0] != "auction"], pane=5), "auction")       # a missing column
    wrong = [(n, "int64", c.to(torch.int64)) if n == "auction" else (n, k, c) for n, k, c in columns]
    refused(_ffi.ERR_UNSUPPORTED, lambda: plan.feed_columns(0, wrong, pane=5), "auction")                                       # a wrong type
    unchanged()
    nulls = torch.ones(rows, dtype=torch.uint8, device="cuda:0")
    nulls[rows // 2] = 0
    if not generic_only:                                 # q5's state ring keeps no validity
        refused(_ffi.ERR_UNSUPPORTED, lambda: plan.feed_columns(0, columns, {"auction": nulls}, pane=5), "NULL")
        unchanged()
    # the same refusals where the pane would have BEGUN: the ring does not advance
    ctx.clean_data_sources()
    state, want = plan.ring_state(), _q5_rows(ctx.execute()[0][0])
    assert state == (5, 1, 2)
    refused(_ffi.ERR_UNSUPPORTED, lambda: plan.feed_columns(0, wrong, pane=6), "auction")
    refused(_ffi.ERR_INVALID, lambda: plan.feed_columns(0, [c for c in columns if c[0] != "auction"], pane=6), "auction")
    unchanged()
    # a pane that a prefetch has pending for the input must be fed first
    ctx.prefetch_data_sources([[host[6]]], pane=6)
    refused(_ffi.ERR_INVALID, lambda: plan.feed_columns(0, *device[6], pane=6))
    unchanged()
    ctx.feed_data_sources(None, pane=6)
    # after all of it the ring still works: panes 5 and 6 are the window
    ref = ExecutionContext([_plan(5)], gpu=gpu, generic_only=generic_only)
    ref.feed_data_sources([[host[1] + host[6]]])
    assert _q5_rows(ctx.execute()[0][0]) == _q5_rows(ref.execute()[0][0])
    ctx.clean_data_sources()
    ctx.feed_device_sources([device[7]], pane=7)
    ref.clean_data_sources()
    ref.feed_data_sources([[host[6] + host[7]]])
    assert _q5_rows(ctx.execute()[0][0]) == _q5_rows(ref.execute()[0][0])
    # ring_close after device panes: feed_columns works again on the same plan
    ctx.close_window_ring()
    assert ctx.feed_device_sources([device[0]]) >= 1
    ref.clean_data_sources()
    ref.feed_data_sources([[host[0]]])
    assert _q5_rows(ctx.execute()[0][0]) == _q5_rows(ref.execute()[0][0])
    ctx.close()
    ref.close()


# ------------------------------------------------------------------ text in, event-time panes, ring, text out
def _csv_rows(text):
    lines = bytes(text.cpu().numpy()).decode().splitlines()
    assert lines[0] == "auction,num"
    return sorted(tuple(int(v) for v in line.split(",")) for line in lines[1:])


@pytest.mark.parametrize("interleave", [False, True])
def test_json_lines_to_event_time_panes_to_the_ring_to_csv(gpu, interleave):
    import torch
    from flock_amd.nexmark import event_bytes_to_columns, event_source
    from flock_amd.runtime import ExecutionContext, device_panes
    n, hops, ppw = 3 * 8_192 + 5, 6, 2
    b = oracle.NexmarkStream(seed=23, eps=9_000).bids(0, 40_000)
    b = {k: v[:n] for k, v in b.items()}
    assert len(b["auction"]) == n
    t = b["b_date_time"]
    origin, hop = int(t[0]), (int(t[-1]) - int(t[0])) // hops + 1
    ids = np.floor_divide(t - origin, hop)
    assert ids[0] == 0 and ids[-1] == hops - 1 and (np.diff(ids) >= 0).all()
    bounds = np.searchsorted(ids, np.arange(hops + 1), side="left")
    host = [[bid_batch(b, int(bounds[p]), int(bounds[p + 1]))] for p in range(hops)]
    if interleave:                                      # the bids of panes 2 and 3, turn by turn: no longer in pane order
        a0, a1, a2 = int(bounds[2]), int(bounds[3]), int(bounds[4])
        m = min(a1 - a0, a2 - a1)
        mixed = np.empty(2 * m, np.int64)
        mixed[0::2], mixed[1::2] = np.arange(a0, a0 + m), np.arange(a1, a1 + m)
        order = np.concatenate([np.arange(a0), mixed, np.arange(a0 + m, a1), np.arange(a1 + m, n)])
        assert sorted(order.tolist()) == list(range(n))
        b = {k: v[order] for k, v in b.items()}
    text = torch.from_numpy(np.frombuffer(oracle.nexmark_json_lines("bid", b), np.uint8).copy()).to("cuda:0")
    cols, rows = event_bytes_to_columns(gpu, text, "bid")
    assert rows == n
    columns, valid = event_source("bid", cols)
    panes = device_panes(gpu, columns, valid, "b_date_time", hop, origin)
    assert [p for p, _, _ in panes] == list(range(hops))
    assert [c[0][2].numel() for _, c, _ in panes] == np.diff(bounds).tolist()
    dev = ExecutionContext([_plan(5)], name="e2e-dev", gpu=gpu)
    ref = ExecutionContext([_plan(5)], name="e2e-host", gpu=gpu)
    dev.open_window_ring(ppw)
    ref.open_window_ring(ppw)
    for p, columns_p, valid_p in panes:
        assert dev.feed_device_sources([(columns_p, valid_p)], pane=p) >= 1
        dev.execute_retain()
        out_cols, out_valid, out_rows = dev.result_columns()
        got = _csv_rows(gpu.csv_encode(out_cols, out_valid))
        dev.clean_data_sources()
        ref.feed_data_sources([[host[p]]], pane=p)
        want = _q5_rows(ref.execute()[0][0])
        ref.clean_data_sources()
        assert len(got) == out_rows and got == want and want, p
    dev.close()
    ref.close()
