"""Device columns into a plan leaf and out of a retained result (flockgpu_plan_feed_columns / flockgpu_plan_result_columns, plan_source.hip), in one process.

Input: the bids of bench.py's arch_ops -- 100 s of NEXMark events at 1e6 events/s, 9.2e7 rows of (auction, bidder, price, b_date_time), 20 bytes a row --
generated on the device.  The plan is a filter + projection that reads all four columns.  Readings, all in this run:
  copy_feed      reset + flockgpu_plan_feed_columns + synchronise, the columns copied behind the (empty) leaf;
  borrow_feed    the same with FLOCKGPU_FEED_BORROW: the leaf reads the generator's tensors in place;
  host_feed      the same rows through flockgpu_plan_feed from registered host memory -- the parent commit's only route into a leaf;
  memcpy_d2d     flockgpu_memcpy device-to-device of the same four columns: the yardstick for the append;
  null_feed      validity bytes on `auction` with 10 % NULLs, a column the filter lets the feed drop rows by: census + row list + tail take;
  end_to_end     serde_json lines of 1.84e7 bids (bench.py's JSON ingest rows) -> decode -> feed -> the q2 plan -> result view -> CSV text, nothing on the host.
Per reading: wall time per call (5 warm-up and 20 timed calls, medians) and every kernel by the library's dispatch-bound events.  The fed leaf is executed
once before anything is timed and its row count compared with numpy's.  Writes one JSON document (default profiles/device_feed/bench.json) and prints it.

    python tools/bench_device_feed.py [--seconds 100] [--eps 1000000] [--steps 20] [--warmup 5] [--out profiles/device_feed/bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_csv import HBM_PEAK, measure  # noqa: E402

TS = {"Timestamp": ["Millisecond", None]}
BID = [("auction", "Int32"), ("bidder", "Int32"), ("price", "Int32"), ("b_date_time", TS)]


def bid_filter_plan(threshold):
    """Projection [auction, bidder, price, b_date_time] over Filter auction >= threshold over the bid scan"""
    fields = [{"data_type": t, "dict_id": 0, "dict_is_ordered": False, "name": n, "nullable": True} for n, t in BID]
    col = lambda k: {"physical_expr": "column", "name": BID[k][0], "index": k}
    scan = {"execution_plan": "memory_exec", "schema": {"fields": fields, "metadata": {}}, "projection": [0, 1, 2, 3]}
    pred = {"physical_expr": "binary_expr", "left": col(0), "op": "GtEq", "right": {"physical_expr": "literal", "value": {"Int32": threshold}}}
    filt = {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096, "input": {"execution_plan": "filter_exec", "predicate": pred, "input": scan}}
    return {"execution_plan": "projection_exec", "expr": [[col(k), BID[k][0]] for k in range(4)], "input": filt, "schema": {"fields": fields, "metadata": {}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--copies", type=int, default=100)
    ap.add_argument("--block-events", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_feed", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    import torch
    from flock_amd import GpuContext, NEXMarkSource, Window, _ffi
    from flock_amd.nexmark import NEXMARK_JSON_SCHEMAS, columns_to_event_bytes, event_source
    from flock_amd.runtime import ExecutionContext
    gpu = GpuContext(0)
    lib = _ffi.load()
    dev = f"cuda:{gpu.device}"
    g = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid",))
    columns, _ = event_source("bid", g.bids)
    rows = columns[0][2].numel()
    nbytes = sum(c.numel() * c.element_size() for _, _, c in columns)
    threshold = int(np.median(g.bids.auction[::97].cpu().numpy()))
    want = int((g.bids.auction >= threshold).sum())
    ctx = ExecutionContext([bid_filter_plan(threshold)], gpu=gpu)
    plan = ctx.plans[0]
    out = {"input": {"bids": rows, "column_bytes": nbytes, "seconds": a.seconds, "eps": a.eps, "filter_keeps": want}, "steps": a.steps, "warmup": a.warmup,
           "hbm_peak_bytes_per_s": HBM_PEAK,
           "recipe": "per call: flockgpu_plan_reset, the feed, a synchronise; wall medians of `steps` calls after `warmup`; kernels from the library's dispatch-bound events "
                     "over the same calls again; hbm_GBps_read_plus_written = 2 x the column bytes / the wall median, pcie_GBps = the column bytes / the wall median; "
                     "borrow_feed moves nothing and has no rate"}

    def reading(call, hbm_bytes=0, pcie_bytes=0):
        """hbm_bytes: column bytes the call reads AND writes in HBM (counted twice); pcie_bytes: bytes it brings over PCIe; neither: nothing moves, no rate"""
        m = measure(torch, gpu, call, a.steps, a.warmup)
        ms = m["wall_ms"]["median"]
        if hbm_bytes or pcie_bytes:
            m["rows_per_s"] = round(rows / (ms * 1e-3), 1)
        if hbm_bytes:
            m["hbm_GBps_read_plus_written"] = round(2 * hbm_bytes / (ms * 1e-3) / 1e9, 1)
        if pcie_bytes:
            m["pcie_GBps"] = round(pcie_bytes / (ms * 1e-3) / 1e9, 1)
        return m

    def device_feed(valid=None, borrow=False):
        def call():
            plan.reset()
            plan.feed_columns(0, columns, valid, borrow=borrow)
            gpu.synchronize()
        return call

    for label, borrow in (("copy_feed", False), ("borrow_feed", True)):
        device_feed(None, borrow)()
        got = plan.execute_retain()
        if got != want:
            raise RuntimeError("%s: %d rows, numpy has %d" % (label, got, want))
        out[label] = reading(device_feed(None, borrow), hbm_bytes=0 if borrow else nbytes)
    plan.reset()

    # ---- the same rows from registered host memory
    host = {name: col.cpu().numpy() for name, _, col in columns}
    regs = [arr.ctypes.data for arr in host.values() if lib.flockgpu_host_register(C.c_void_p(arr.ctypes.data), arr.nbytes) == 0]
    rb = pa.record_batch([pa.array(host[n]).cast(pa.timestamp("ms")) if n == "b_date_time" else pa.array(host[n]) for n, _ in BID], names=[n for n, _ in BID])

    def host_feed():
        plan.reset()
        plan.feed(0, [rb])
        gpu.synchronize()
    host_feed()
    got = plan.execute_retain()
    if got != want:
        raise RuntimeError("host_feed: %d rows, numpy has %d" % (got, want))
    out["host_feed"] = reading(host_feed, pcie_bytes=nbytes)
    out["host_feed"]["registered_columns"] = len(regs)
    plan.reset()
    for ptr in regs:
        lib.flockgpu_host_unregister(C.c_void_p(ptr))
    del host, rb

    # ---- the yardstick: a plain device-to-device copy of the same bytes
    twins = [torch.empty_like(col) for _, _, col in columns]

    def memcpy_d2d():
        for (_, _, col), twin in zip(columns, twins):
            gpu._check(lib.flockgpu_memcpy(gpu._h, twin.data_ptr(), col.data_ptr(), col.numel() * col.element_size(), _ffi.D2D))
    out["memcpy_d2d"] = reading(memcpy_d2d, hbm_bytes=nbytes)
    del twins

    # ---- 10 % NULLs in the column the filter compares: census + compaction
    torch.manual_seed(5)
    ok = (torch.rand(rows, device=dev) >= 0.1).to(torch.uint8)
    want_nulls = int(((g.bids.auction >= threshold) & (ok != 0)).sum())
    device_feed({"auction": ok})()
    got = plan.execute_retain()
    if got != want_nulls:
        raise RuntimeError("null_feed: %d rows, numpy has %d" % (got, want_nulls))
    out["null_feed"] = reading(device_feed({"auction": ok}), hbm_bytes=nbytes)
    out["null_feed"]["rows_dropped_at_the_feed"] = bool("take_tail_kernel" in out["null_feed"]["kernels"])
    plan.reset()
    ctx.close()
    del ok, columns, g

    # ---- text -> decode -> plan -> encode -> text
    block = NEXMarkSource(1, a.block_events, Window.element_wise(), seed=20260926).generate_data(gpu, relations=("bid",)).bids
    bids = {k: getattr(block, k).repeat(a.copies) for k in ("auction", "bidder", "price", "b_date_time")}
    text = columns_to_event_bytes(gpu, "bid", bids)
    n_text = bids["auction"].numel()
    q2 = ExecutionContext([open(os.path.join(ROOT, "tests", "golden", "plans", "q2.json")).read()], gpu=gpu)
    result = {}

    def end_to_end():
        q2.clean_data_sources()
        cols, n = gpu.json_lines_decode(text, NEXMARK_JSON_SCHEMAS["bid"], borrow=True)     # (event_bytes_to_columns, its columns borrowed)
        q2.feed_device_sources([event_source("bid", cols)])
        result["rows"] = q2.execute_retain()[0]
        result["text"] = gpu.csv_encode(*q2.result_columns()[:2], borrow=True)
        gpu.synchronize()
    end_to_end()
    want_q2 = int((bids["auction"] % 123 == 0).sum())
    if result["rows"] != want_q2 or int((result["text"] == 10).sum()) != want_q2 + 1:
        raise RuntimeError("end_to_end: %d rows, numpy has %d" % (result["rows"], want_q2))
    m = measure(torch, gpu, end_to_end, a.steps, a.warmup)
    m.update({"rows_in": n_text, "json_bytes_in": int(text.numel()), "rows_out": want_q2, "csv_bytes_out": int(result["text"].numel()),
              "rows_per_s": round(n_text / (m["wall_ms"]["median"] * 1e-3), 1), "plan": "q%d" % q2.plans[0].query})
    out["end_to_end"] = m
    q2.close()
    gpu.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
