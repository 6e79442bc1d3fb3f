"""Scalar functions in expressions (valprog.hpp A-F1..A-F8) on the inputs of bench.py's arch_ops: 100 s of NEXMark events at 1e6 events/s -- 9.2e7 bids,
and 6e6 auctions whose description is 50-99 bytes (~450 MB).  Each workload is planned once, fed once, executed once untimed and ten times timed with its
result kept in HBM (flockgpu_plan_execute_retain); reported per workload: ms per execute as min / median / max, the result's row count and a sum checked
against numpy / pyarrow, and per kernel of interest its time, algorithmic bytes and fraction of the 8 TB/s HBM peak -- next to a yardstick measured by
this tool IN THE SAME PROCESS.  Kernel times here come from the library's dispatch-bound events; a `rocprofv3 --kernel-trace --stats` run of this tool
(no other tracing with it) supplies the profiler's.  Writes profiles/scalar_functions/bench.json (or --out).

  row               statement                                                               yardstick
  Y-project         SELECT price * 2 + 1                              (bench.py expr_project)
  Y-filter          WHERE price / 100 > 5 AND auction % 7 = 1         (bench.py expr_filter)
  Y-contains        WHERE description LIKE '%<needle>%'               (strmatch_contains_kernel)
  SF-floor          SELECT floor(CAST(price AS Float64) / 100.0)                              Y-project
  X-fdiv            SELECT CAST(price AS Float64) / 100.0             (no function: the IEEE division alone)      Y-project
  SF-floor-nodiv    SELECT floor(CAST(price AS Float64) * 0.5)        (the function without the division)         Y-project
  SF-trunc-minute   SELECT date_trunc('minute', b_date_time)                                  Y-project
  SF-trunc-month    SELECT date_trunc('month', b_date_time)                                   Y-project (tens of integer operations per row more)
  SF-hour-filter    WHERE date_part('hour', b_date_time) BETWEEN 8 AND 18                     Y-filter
  SF-bucket         SELECT date_trunc('minute', b_date_time), COUNT(*) GROUP BY 1             reported only
  SF-charlen        WHERE char_length(description) > 80                                       Y-contains

Algorithmic bytes: the columns an expression reads once plus what it writes once (a projection of an Int32: 4 in + 8 out per row; of a Timestamp: 8 + 8;
a filter: its columns in, flag words aside); utf8_chars_kernel: the offsets 4 (R + 1), the column's bytes and 4 R of lengths out."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
TS = {"Timestamp": ["Millisecond", None]}


def field(name, dt, nullable=False):
    return {"data_type": dt, "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


BID = [field("auction", "Int32"), field("price", "Int32"), field("b_date_time", TS)]
AUC = [field("a_id", "Int32"), field("description", "Utf8")]


def col(fields, name):
    return {"physical_expr": "column", "name": name, "index": [f["name"] for f in fields].index(name)}


def lit(kind, v):
    return {"physical_expr": "literal", "value": {kind: v}}


def binop(l, op, r):
    return {"physical_expr": "binary_expr", "left": l, "op": op, "right": r}


def cast(e, t):
    return {"physical_expr": "cast_expr", "expr": e, "cast_type": t}


def fn(name, rt, *args):
    return {"physical_expr": "scalar_function_expr", "name": name, "args": list(args), "return_type": rt}


def scan(fields):
    return {"execution_plan": "memory_exec", "schema": {"fields": fields, "metadata": {}}, "projection": list(range(len(fields)))}


def project(fields, e, dt):
    return {"execution_plan": "projection_exec", "expr": [[e, "x"]], "input": scan(fields), "schema": {"fields": [field("x", dt, True)], "metadata": {}}}


def filt(fields, pred, keep):
    f = {"execution_plan": "filter_exec", "predicate": pred, "input": scan(fields)}
    return {"execution_plan": "projection_exec", "expr": [[col(fields, k), k] for k in keep], "input": f,
            "schema": {"fields": [x for x in fields if x["name"] in keep], "metadata": {}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scalar_functions", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    import pyarrow.compute as pc
    from flock_amd import GpuContext, NEXMarkSource, Window
    from flock_amd.runtime import ExecutionContext

    gpu = GpuContext(0)
    g = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid",))
    b = g.bids
    auction, price, when = b.auction.cpu().numpy(), b.price.cpu().numpy(), b.b_date_time.cpu().numpy()
    del g, b
    bid_rb = pa.record_batch([pa.array(auction), pa.array(price), pa.array(when).cast(pa.timestamp("ms"))], names=[f["name"] for f in BID])
    n_bid = len(price)
    rng = np.random.default_rng(11)
    n_auc = a.seconds * a.eps // 50 * 3
    lens = rng.integers(50, 100, n_auc).astype(np.int32)
    off = np.zeros(n_auc + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    data = rng.integers(97, 123, int(off[-1]), dtype=np.uint8)
    desc = pa.StringArray.from_buffers(n_auc, pa.py_buffer(off.tobytes()), pa.py_buffer(data.tobytes()))
    auc_rb = pa.record_batch([pa.array(np.arange(n_auc, dtype=np.int32)), desc], names=[f["name"] for f in AUC])
    needle = desc[12345].as_py()[20:23]

    i64 = lambda e: cast(e, "Int64")
    unit = lambda u: lit("Utf8", u)
    t_col, p_col, a_col = col(BID, "b_date_time"), col(BID, "price"), col(BID, "auction")
    hour = fn("date_part", "Int32", unit("hour"), t_col)
    minute = fn("date_trunc", TS, unit("minute"), t_col)
    key = "datetrunc(Utf8(\"minute\"),b_date_time)"
    cnt = [{"aggregate_expr": "count", "name": "COUNT(UInt8(1))", "data_type": "UInt64", "nullable": True, "expr": lit("UInt8", 1)}]
    bucket = {"execution_plan": "hash_aggregate_exec", "mode": "Final", "group_expr": [[{"physical_expr": "column", "name": key, "index": 0}, key]], "aggr_expr": cnt,
              "schema": {"fields": [field(key, TS, True), field("COUNT(UInt8(1))", "UInt64", True)], "metadata": {}}, "input_schema": {"fields": BID, "metadata": {}},
              "input": {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [[minute, key]], "aggr_expr": cnt, "input": scan(BID),
                        "schema": {"fields": [field(key, TS, True), field("COUNT(UInt8(1))[count]", "UInt64", True)], "metadata": {}}, "input_schema": {"fields": BID, "metadata": {}}}}
    hours = ((when // 3_600_000) % 24).astype(np.int64)
    in_hours = (hours >= 8) & (hours <= 18)
    y_filter = (price.astype(np.int64) // 100 > 5) & (auction.astype(np.int64) % 7 == 1)
    chars = pc.utf8_length(desc).to_numpy()
    # name: (plan, feed, kernel of interest, algorithmic bytes, yardstick row, check(result batch, rows))
    W = {
        "Y-project": (project(BID, binop(binop(i64(p_col), "Multiply", lit("Int64", 2)), "Plus", lit("Int64", 1)), "Int64"), bid_rb, "valprog_kernel", 12.0 * n_bid, None,
                      lambda rb: (int(pc.sum(rb.column(0)).as_py()), int((price.astype(np.int64) * 2 + 1).sum()))),
        "Y-filter": (filt(BID, binop(binop(binop(i64(p_col), "Divide", lit("Int64", 100)), "Gt", lit("Int64", 5)), "And", binop(binop(i64(a_col), "Modulo", lit("Int64", 7)), "Eq", lit("Int64", 1))),
                          ["auction", "price"]), bid_rb, "valprog_kernel", 8.0 * n_bid, None,
                     lambda rb: ((rb.num_rows, int(pc.sum(rb.column(1)).as_py())), (int(y_filter.sum()), int(price[y_filter].astype(np.int64).sum())))),
        "Y-contains": (filt(AUC, binop(col(AUC, "description"), "Like", lit("Utf8", "%" + needle + "%")), ["a_id"]), auc_rb, "strmatch_contains_kernel",
                       4.0 * (n_auc + 1) + len(data) + 4.0 * n_auc / 32, None,
                       lambda rb: (rb.num_rows, int(pc.sum(pc.match_substring(desc, needle)).as_py()))),
        "SF-floor": (project(BID, fn("floor", "Float64", binop(cast(p_col, "Float64"), "Divide", lit("Float64", 100.0))), "Float64"), bid_rb, "valprog_kernel", 12.0 * n_bid, "Y-project",
                     lambda rb: (float(pc.sum(rb.column(0)).as_py()), float(np.floor(price.astype(np.float64) / 100.0).sum()))),
        # (two rows that take SF-floor apart: the Float64 division without the function, the function without the division)
        "X-fdiv": (project(BID, binop(cast(p_col, "Float64"), "Divide", lit("Float64", 100.0)), "Float64"), bid_rb, "valprog_kernel", 12.0 * n_bid, "Y-project",
                   lambda rb: (bool(np.array_equal(rb.column(0).to_numpy(), price.astype(np.float64) / 100.0)), True)),      # (every quotient, bit for bit)
        "SF-floor-nodiv": (project(BID, fn("floor", "Float64", binop(cast(p_col, "Float64"), "Multiply", lit("Float64", 0.5))), "Float64"), bid_rb, "valprog_kernel", 12.0 * n_bid, "Y-project",
                           lambda rb: (float(pc.sum(rb.column(0)).as_py()), float(np.floor(price.astype(np.float64) * 0.5).sum()))),
        "SF-trunc-minute": (project(BID, minute, TS), bid_rb, "valprog_kernel", 16.0 * n_bid, "Y-project",
                            lambda rb: (int(pc.sum(rb.column(0).cast(pa.int64())).as_py()), int((when // 60_000 * 60_000).sum()))),
        "SF-trunc-month": (project(BID, fn("date_trunc", TS, unit("month"), t_col), TS), bid_rb, "valprog_kernel", 16.0 * n_bid, "Y-project",
                           lambda rb: (int(pc.sum(rb.column(0).cast(pa.int64())).as_py()),
                                       int(pc.sum(pc.floor_temporal(bid_rb.column(2), unit="month").cast(pa.int64())).as_py()))),
        "SF-hour-filter": (filt(BID, binop(binop(hour, "GtEq", lit("Int32", 8)), "And", binop(hour, "LtEq", lit("Int32", 18))), ["auction", "price"]), bid_rb, "valprog_kernel",
                           8.0 * n_bid, "Y-filter", lambda rb: ((rb.num_rows, int(pc.sum(rb.column(1)).as_py() or 0)), (int(in_hours.sum()), int(price[in_hours].astype(np.int64).sum())))),
        "SF-bucket": (bucket, bid_rb, "valprog_kernel", 16.0 * n_bid, None,
                      lambda rb: ((rb.num_rows, int(pc.sum(rb.column(1)).as_py())), (len(np.unique(when // 60_000)), n_bid))),
        "SF-charlen": (filt(AUC, binop(fn("char_length", "Int32", col(AUC, "description")), "Gt", lit("Int32", 80)), ["a_id"]), auc_rb, "utf8_chars_kernel",
                       4.0 * (n_auc + 1) + len(data) + 4.0 * n_auc, "Y-contains", lambda rb: (rb.num_rows, int((chars > 80).sum()))),
    }
    out = {"input": {"bids": int(n_bid), "auctions": int(n_auc), "description_bytes": int(len(data)), "seconds": a.seconds, "eps": a.eps}, "executes": a.executes,
           "recipe": "plan once, feed once, one untimed and N timed executes with the result retained in HBM; kernel times from the library's dispatch-bound events"}
    failed = False
    for name, (plan, rb, kernel, alg, yard, check) in W.items():
        if a.only and name not in a.only.split(","):
            continue
        e = {"yardstick": yard}
        ctx = ExecutionContext([plan], gpu=gpu, generic_only=True)
        try:
            ctx.feed_data_sources([[[rb]]])
            pl = ctx.plans[0]
            got, want = check(ctx.execute()[0][0])      # (the untimed execute: arena growth; its result is checked)
            if got != want:
                raise RuntimeError(f"{name}: result {got}, numpy / pyarrow say {want}")
            gpu.synchronize()
            times = []
            for _ in range(a.executes):
                t0 = time.perf_counter()
                rows = pl.execute_retain()
                gpu.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            gpu.profile_reset()
            gpu.profile_only(None)
            gpu.profile(True)
            for _ in range(4):
                pl.execute_retain()
            gpu.synchronize()
            stats = gpu.profile_read()
            gpu.profile(False)
            e.update({"result_rows": int(rows), "checked": [str(x) for x in (got if isinstance(got, tuple) else (got,))],
                      "ms_per_execute": {"min": round(min(times), 4), "median": round(statistics.median(times), 4), "max": round(max(times), 4)},
                      "kernels_ms_per_execute": {k: round(v["total_ms"] / 4, 4) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])[:6]}})
            st = stats.get(kernel)
            if st and st["launches"]:
                ms = st["total_ms"] / 4
                e["kernel"] = {"name": kernel, "ms_per_execute": round(ms, 4), "launches_per_execute": st["launches"] / 4, "algorithmic_bytes": int(alg),
                               "GB_per_s": round(alg / (ms * 1e-3) / 1e9, 1), "frac_of_hbm_peak": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
                if yard and "kernel" in out.get(yard, {}):
                    e["yardstick_frac_of_hbm_peak"] = out[yard]["kernel"]["frac_of_hbm_peak"]
                    e["yardstick_kernel_ms"] = out[yard]["kernel"]["ms_per_execute"]
        except Exception as ex:   # (a workload that fails is reported, the others still run)
            e["error"] = repr(ex)
            failed = True
        finally:
            ctx.close()
        out[name] = e
        print(name, json.dumps(e), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    gpu.close()
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
