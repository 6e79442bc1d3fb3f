"""Aggregate window functions (relops.hpp window_aggregates, window.hip) on the inputs of bench.py's arch_ops: 100 s of NEXMark events at 1e6
events/s (9.2e7 bids).  Each workload (a sort_exec on its PARTITION BY / ORDER BY under a window_agg_exec) is planned once, fed once and executed 10
times with its result kept in HBM (flockgpu_plan_execute_retain); reported per workload: ms per execute, kernel launches per execute, the window node's
own kernel time apart from the sort below it, and per new kernel its time, algorithmic bytes and fraction of the 8 TB/s HBM peak.  Writes
profiles/window_aggregates/bench.json (or --out).

Host waits per execute (--host-waits): as tools/bench_composite_keys.py -- two child runs under `rocprofv3 --hip-trace --stats` with 2 and 7
executes; the difference of their blocking HIP calls over the 5 extra executes, less the timing loop's own synchronisation, per execute.  The
sort below the window waits on its key ranges; run --only with a workload to see its own count.

Algorithmic bytes per row (k: key bytes, a: argument bytes, o: output bytes with validity): win_tile_kernel k + a (+ 2/8 for the flag words it
writes); win_emit_kernel a + o (+ 2/8 flag words read); win_carry_kernel reads and writes per-tile summaries only (not counted).  The window node
as a whole: k + a + o -- what a single pass that reads every input once and writes every output once would move.

Workloads:
  a   MAX(price) OVER (PARTITION BY auction ORDER BY b_date_time)
  b   COUNT(*), SUM(price) OVER (PARTITION BY bidder)
  c   COUNT(*) OVER (ORDER BY b_date_time)           (one partition over every tile; many bids share a millisecond)
  d   ROW_NUMBER() OVER (PARTITION BY auction ORDER BY b_date_time)    (a's sort: the yardstick)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
TS = {"Timestamp": ["Millisecond", None]}


def field(name, dt):
    return {"data_type": dt, "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": False}


BID = [field("auction", "Int32"), field("bidder", "Int32"), field("price", "Int32"), field("b_date_time", TS)]


def col(fields, name):
    return {"physical_expr": "column", "name": name, "index": [f["name"] for f in fields].index(name)}


def scan(fields):
    return {"execution_plan": "memory_exec", "schema": {"fields": fields, "metadata": {}}, "projection": list(range(len(fields)))}


def window_plan(sort_keys, part, order, entries):
    asc = {"descending": False, "nulls_first": False}
    srt = {"execution_plan": "sort_exec", "input": scan(BID), "expr": [{"expr": col(BID, k), "options": asc} for k in sort_keys]}
    out = []
    for fn, arg, dt, name in entries:
        if fn == "row_number":
            out.append({"window_expr": "built_in_window_expr", "fun": "RowNumber", "name": name, "partition_by": [col(BID, p) for p in part], "order_by": []})
            continue
        e = {"aggregate_expr": fn, "name": name, "data_type": dt, "nullable": True,
             "expr": col(BID, arg) if arg else {"physical_expr": "literal", "value": {"UInt8": 1}}}
        out.append({"window_expr": "aggregate_window_expr", "aggregate": e, "partition_by": [col(BID, p) for p in part],
                    "order_by": [{"expr": col(BID, o), "options": asc} for o in order]})
    return {"execution_plan": "window_agg_exec", "input": srt, "window_expr": out}


def workloads():
    """name -> (plan, key bytes per row, argument bytes per row, output bytes per row)"""
    return {
        "a": (window_plan(["auction", "b_date_time"], ["auction"], ["b_date_time"], [("max", "price", "Int32", "best")]), 12.0, 4.0, 5.0),
        "b": (window_plan(["bidder"], ["bidder"], [], [("count", None, "UInt64", "n"), ("sum", "price", "Int64", "total")]), 4.0, 4.0, 17.0),
        "c": (window_plan(["b_date_time"], [], ["b_date_time"], [("count", None, "UInt64", "n")]), 8.0, 0.0, 8.0),
        "d": (window_plan(["auction", "b_date_time"], ["auction"], [], [("row_number", None, None, "rn")]), 4.0, 0.0, 8.0),
    }


WAIT_CALLS = ("hipStreamSynchronize", "hipEventSynchronize", "hipDeviceSynchronize", "hipMemcpy", "hipMemcpyWithStream", "hipMemcpyDtoH", "hipMemcpyHtoD")


def host_waits(name):
    """Blocking HIP calls per execute of workload `name` (see the module docstring): two child runs under rocprofv3."""
    import csv
    import glob
    import subprocess
    import tempfile
    counts = {}
    for n_exec in (2, 7):
        d = tempfile.mkdtemp(prefix="wa_waits_")
        cmd = ["rocprofv3", "--hip-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--only", name, "--executes", str(n_exec), "--out", os.path.join(d, "child.json")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        total = 0
        for f in glob.glob(os.path.join(d, "**", "*hip_api_stats.csv"), recursive=True):
            with open(f) as fh:
                for row in csv.DictReader(fh):
                    if row["Name"] in WAIT_CALLS:
                        total += int(row["Calls"])
        counts[n_exec] = total
    return {"per_execute": round((counts[7] - counts[2]) / 5 - 1, 2), "blocking_calls_at_2_and_7_executes": [counts[2], counts[7]]}


NEW_KERNELS = ("win_tile_kernel", "win_carry_kernel", "win_emit_kernel")
ROW_NUMBER_KERNELS = ("run_start_kernel", "run_first_kernel", "run_rank_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_aggregates", "bench.json"))
    ap.add_argument("--host-waits", action="store_true", help="also count blocking HIP calls per execute (child runs under rocprofv3)")
    a = ap.parse_args()
    waits = {}
    if a.host_waits:   # (before this process opens the GPU: the children generate their own inputs)
        for name in workloads():
            if not a.only or name in a.only.split(","):
                waits[name] = host_waits(name)
                print(name, "host waits", waits[name], flush=True)
    import pyarrow as pa
    from flock_amd import GpuContext, NEXMarkSource, Window
    from flock_amd.runtime import ExecutionContext

    gpu = GpuContext(0)
    src = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid",))
    b = src.bids
    bid_rb = pa.record_batch([pa.array(b.auction.cpu().numpy()), pa.array(b.bidder.cpu().numpy()), pa.array(b.price.cpu().numpy()),
                              pa.array(b.b_date_time.cpu().numpy()).cast(pa.timestamp("ms"))], names=[f["name"] for f in BID])
    del src, b
    n = bid_rb.num_rows
    out = {"input": {"bids": n, "seconds": a.seconds, "eps": a.eps}, "executes": a.executes,
           "recipe": "plan once, feed once, executes with the result retained in HBM; kernel times from the library's dispatch-bound events"}
    for name, (plan, kb, ab, ob) in workloads().items():
        if a.only and name not in a.only.split(","):
            continue
        ctx = ExecutionContext([plan], gpu=gpu)
        e = {}
        try:
            ctx.feed_data_sources([[[bid_rb]]])
            pl = ctx.plans[0]
            rows = pl.execute_retain()      # (first execute: statistics, arena growth)
            gpu.synchronize()
            times = []
            for _ in range(a.executes):
                t0 = time.perf_counter()
                rows = pl.execute_retain()
                gpu.synchronize()
                times.append(time.perf_counter() - t0)
            gpu.profile_reset()
            gpu.profile_only(None)
            gpu.profile(True)
            for _ in range(2):
                pl.execute_retain()
            gpu.synchronize()
            stats = gpu.profile_read()
            gpu.profile(False)
            win = NEW_KERNELS + ROW_NUMBER_KERNELS   # the window node's own kernels (ROW_NUMBER's run scan shares its kernels' names with the sort's)
            win_ms = sum(v["total_ms"] for k, v in stats.items() if k in win) / 2
            win_launches = sum(v["launches"] for k, v in stats.items() if k in win) / 2
            e = {"ms_per_execute": round(sum(times) / len(times) * 1e3, 4), "ms_min": round(min(times) * 1e3, 4), "result_rows": int(rows), "input_rows": int(n),
                 "launches_per_execute": sum(v["launches"] for v in stats.values()) / 2,
                 "window_node": {"ms_per_execute": round(win_ms, 4), "launches_per_execute": win_launches},
                 "below_window_ms_per_execute": round(sum(v["total_ms"] for k, v in stats.items() if k not in win) / 2, 4),
                 "kernels_ms_per_execute": {k: round(v["total_ms"] / 2, 4) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])[:12]}}
            if name in waits:
                e["host_waits"] = waits[name]
            new = {}
            for k in NEW_KERNELS:
                st = stats.get(k)
                if not st or not st["launches"]:
                    continue
                ms = st["total_ms"] / 2
                alg = {"win_tile_kernel": (kb + ab + 0.25) * n, "win_carry_kernel": 0.0, "win_emit_kernel": (ab + ob + 0.25) * n}[k]
                new[k] = {"ms_per_execute": round(ms, 4), "algorithmic_bytes": int(alg), "GB_per_s": round(alg / (ms * 1e-3) / 1e9, 1),
                          "frac_of_hbm_peak": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
            e["new_kernels"] = new
            if new:
                ms = sum(v["ms_per_execute"] for v in new.values())
                alg = (kb + ab + ob) * n
                e["segmented_scan"] = {"ms_per_execute": round(ms, 4), "algorithmic_bytes": int(alg), "GB_per_s": round(alg / (ms * 1e-3) / 1e9, 1),
                                       "frac_of_hbm_peak": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        except Exception as ex:   # (a workload that fails is reported, the others still run)
            e = {"error": repr(ex)}
        ctx.close()
        out[name] = e
        print(name, json.dumps(e), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else v.get("ms_per_execute", v.get("error"))) for k, v in out.items() if k != "input"}))
    gpu.close()


if __name__ == "__main__":
    main()
