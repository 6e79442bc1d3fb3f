"""Composite-key GROUP BY / join (relops.hpp key_codes) on the inputs of bench.py's arch_ops: 100 s of NEXMark events at 1e6 events/s (9.2e7 bids,
the auctions beside them).  Each workload is planned once, fed once and executed 10 times with its result kept in HBM
(flockgpu_plan_execute_retain); reported per workload: ms per execute, kernel launches per execute, and per new kernel its time, algorithmic
bytes and fraction of the 8 TB/s HBM peak.  Writes profiles/composite_keys/bench.json (or --out).

Host waits per execute (--host-waits): the library's kernel timer does not see them, so every workload also runs in two child processes of this
tool under `rocprofv3 --hip-trace --stats`, with 2 and 7 executes; the difference of their blocking HIP calls (stream / event / device
synchronisations, synchronous copies) over the 5 extra executes, less the one stream synchronisation the timing loop itself makes per execute, is
the workload's waits per execute.

Algorithmic bytes of the new kernels (R build rows, G groups of the build side, P probe rows, kb / kp key bytes per build / probe row -- Utf8: its
bytes + its offset): insert (kb + 4) R (keys in, slot out); first 9 R (slot in, first row out, flag out); rank 8 G (first row in, id out);
gid 4 R + 8 (R - G) (first row in; a row that is not its group's first reads that row's id and writes its own); probe (kp + 4) P.  Table slots
are not counted: they are the pass's overhead.

Workloads:
  G-hi    GROUP BY auction, bidder, price; COUNT(*), MAX(b_date_time)      (about one group per row)
  G-ref   GROUP BY auction, bidder;        COUNT(*), MAX(b_date_time)      (today's packed Int32 pair: the yardstick of G-hi)
  G-lo    GROUP BY bidder % 64, auction % 32, price % 8; COUNT(*), SUM(price)  (at most 16384 groups)
  G-utf8  GROUP BY item_name, category over the auctions
  J       bid JOIN auction ON auction = a_id AND bidder = seller AND b_date_time = a_date_time
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
AUC = [field("a_id", "Int32"), field("item_name", "Utf8"), field("a_date_time", TS), field("seller", "Int32"), field("category", "Int32")]


def col(fields, name):
    return {"physical_expr": "column", "name": name, "index": [f["name"] for f in fields].index(name)}


def scan(fields):
    return {"execution_plan": "memory_exec", "schema": {"fields": fields, "metadata": {}}, "projection": list(range(len(fields)))}


def modulo(fields, name, m):
    return {"physical_expr": "binary_expr", "op": "Modulo", "left": col(fields, name), "right": {"physical_expr": "literal", "value": {"Int32": m}}}


def agg(fn, arg, dt, name):
    return {"aggregate_expr": fn, "name": name, "data_type": dt, "nullable": True, "expr": arg}


def group_plan(fields, group, aggs):
    return {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": group, "aggr_expr": aggs, "input": scan(fields),
            "input_schema": {"fields": fields, "metadata": {}}, "schema": {"fields": [], "metadata": {}}}


def workloads():
    one = {"physical_expr": "literal", "value": {"UInt8": 1}}
    cnt = agg("count", one, "UInt64", "COUNT(UInt8(1))")
    mx = agg("max", col(BID, "b_date_time"), TS, "MAX(b_date_time)")
    g = lambda names: [[col(BID, n), n] for n in names]
    return {
        "G-hi": (group_plan(BID, g(["auction", "bidder", "price"]), [cnt, mx]), "bid", 12.0),
        "G-ref": (group_plan(BID, g(["auction", "bidder"]), [cnt, mx]), "bid", 8.0),
        "G-lo": (group_plan(BID, [[modulo(BID, "bidder", 64), "b64"], [modulo(BID, "auction", 32), "a32"], [modulo(BID, "price", 8), "p8"]],
                            [cnt, agg("sum", col(BID, "price"), "Int64", "SUM(price)")]), "bid", 12.0),
        "G-utf8": (group_plan(AUC, [[col(AUC, "item_name"), "item_name"], [col(AUC, "category"), "category"]], [cnt]), "auction", None),
        "J": ({"execution_plan": "hash_join_exec", "left": scan(BID), "right": scan(AUC), "join_type": "Inner", "mode": "CollectLeft",
               "on": [[col(BID, "auction"), col(AUC, "a_id")], [col(BID, "bidder"), col(AUC, "seller")], [col(BID, "b_date_time"), col(AUC, "a_date_time")]],
               "schema": {"fields": BID + AUC, "metadata": {}}}, "both", None),
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
        d = tempfile.mkdtemp(prefix="ck_waits_")
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


NEW_KERNELS = ("key_codes_insert_kernel", "key_codes_first_kernel", "key_codes_rank_kernel", "key_codes_gid_kernel", "key_codes_probe_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_keys", "bench.json"))
    ap.add_argument("--host-waits", action="store_true", help="also count blocking HIP calls per execute (child runs under rocprofv3)")
    a = ap.parse_args()
    waits = {}
    if a.host_waits:   # (before this process opens the GPU: the children generate their own inputs)
        for name in workloads():
            if not a.only or name in a.only.split(","):
                waits[name] = host_waits(name)
                print(name, "host waits", waits[name], flush=True)
    import numpy as np
    import pyarrow as pa
    from flock_amd import GpuContext, NEXMarkSource, Window
    from flock_amd.runtime import ExecutionContext

    gpu = GpuContext(0)
    src = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid", "auction"), auction_times=True)
    b, au = src.bids, src.auctions
    ts = pa.timestamp("ms")
    rng = np.random.default_rng(11)
    lens = rng.integers(8, 20, au.rows).astype(np.int32)          # item_name at the widths of the reference's generator (up to 19 bytes)
    off = np.zeros(au.rows + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    text = rng.integers(97, 100, int(off[-1]), dtype=np.uint8)    # (a three-letter alphabet: names repeat, the GROUP BY has groups to find)
    names = pa.StringArray.from_buffers(au.rows, pa.py_buffer(off.tobytes()), pa.py_buffer(text.tobytes()))
    bid_rb = pa.record_batch([pa.array(b.auction.cpu().numpy()), pa.array(b.bidder.cpu().numpy()), pa.array(b.price.cpu().numpy()),
                              pa.array(b.b_date_time.cpu().numpy()).cast(ts)], names=[f["name"] for f in BID])
    auc_rb = pa.record_batch([pa.array(au.a_id.cpu().numpy()), names, pa.array(au.a_date_time.cpu().numpy()).cast(ts), pa.array(au.seller.cpu().numpy()),
                              pa.array(au.category.cpu().numpy())], names=[f["name"] for f in AUC])
    del src, b, au
    n_bids, n_auc = bid_rb.num_rows, auc_rb.num_rows
    out = {"input": {"bids": n_bids, "auctions": n_auc, "seconds": a.seconds, "eps": a.eps}, "executes": a.executes,
           "recipe": "plan once, feed once, executes with the result retained in HBM; kernel times from the library's dispatch-bound events"}
    for name, (plan, rel, key_bytes_per_row) in workloads().items():
        if a.only and name not in a.only.split(","):
            continue
        ctx = ExecutionContext([plan], gpu=gpu)
        e = {}
        try:
            feed = [[[bid_rb]], [[auc_rb]]] if rel == "both" else [[[bid_rb if rel == "bid" else auc_rb]]]
            ctx.feed_data_sources(feed)
            pl = ctx.plans[0]
            rows = pl.execute_retain()      # (first execute: statistics, table sizing, arena growth)
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
            n_in = n_bids if rel == "bid" else n_auc if rel == "auction" else n_bids + n_auc
            e = {"ms_per_execute": round(sum(times) / len(times) * 1e3, 4), "ms_min": round(min(times) * 1e3, 4), "result_rows": int(rows), "input_rows": int(n_in),
                 "launches_per_execute": sum(v["launches"] for v in stats.values()) / 2,
                 "kernels_ms_per_execute": {k: round(v["total_ms"] / 2, 4) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])[:10]}}
            if name in waits:
                e["host_waits"] = waits[name]
            # the build side of key_codes (a join's ids go on its smaller side, the auctions; the bids probe) and its group count
            if rel == "both":
                R, P, kb, kp = n_auc, n_bids, 16.0, 16.0
                keys = np.stack([auc_rb.column("a_id").to_numpy().astype(np.int64), auc_rb.column("seller").to_numpy().astype(np.int64),
                                 auc_rb.column("a_date_time").cast(pa.int64()).to_numpy()], axis=1)
                G = len(np.unique(keys, axis=0))
            else:
                R, P, G = n_in, 0, int(rows)
                kb = key_bytes_per_row if key_bytes_per_row else 8.0 + auc_rb.column("item_name").buffers()[2].size / n_auc   # (offset + bytes + category)
                kp = 0.0
            e["key_codes_rows"] = {"build": int(R), "groups": int(G), "probe": int(P), "build_key_bytes_per_row": round(kb, 3)}
            new = {}
            for k in NEW_KERNELS:
                st = stats.get(k)
                if not st or not st["launches"]:
                    continue
                ms = st["total_ms"] / 2
                alg = {"key_codes_insert_kernel": (kb + 4.0) * R, "key_codes_first_kernel": 9.0 * R, "key_codes_rank_kernel": 8.0 * G,
                       "key_codes_gid_kernel": 4.0 * R + 8.0 * (R - G), "key_codes_probe_kernel": (kp + 4.0) * P}[k]
                new[k] = {"ms_per_execute": round(ms, 4), "algorithmic_bytes": int(alg), "GB_per_s": round(alg / (ms * 1e-3) / 1e9, 1),
                          "frac_of_hbm_peak": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
            e["new_kernels"] = new
        except Exception as ex:   # (a workload that fails is reported, the others still run)
            e = {"error": repr(ex)}
        ctx.close()
        out[name] = e
        print(name, json.dumps(e), flush=True)
    if "G-hi" in out and "G-ref" in out and "ms_per_execute" in out["G-hi"] and "ms_per_execute" in out["G-ref"]:
        out["G-hi_over_G-ref"] = round(out["G-hi"]["ms_per_execute"] / out["G-ref"]["ms_per_execute"], 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else v.get("ms_per_execute", v.get("error"))) for k, v in out.items() if k != "input"}))
    gpu.close()


if __name__ == "__main__":
    main()
