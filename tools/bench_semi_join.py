"""Semi / anti joins (HashJoinExec join_type Semi / Anti, relops.hpp semi_rows) on the inputs of bench.py's arch_ops: 100 s of NEXMark events at
1e6 events/s -- 9.2e7 bids, 6e6 auctions.  Each workload is planned once, fed once and executed 10 times with its result kept in HBM
(flockgpu_plan_execute_retain); reported per workload: min / median / max ms per execute, kernel launches per execute, the kernels' times, and for the
probe kernel its algorithmic bytes (4 per left key + 4 per 32 rows of flag words) as a fraction of the 8 TB/s HBM peak and of the stream yardstick.
Writes profiles/semi_join/bench.json (or --out).

Yardsticks, measured by this tool in the same process: pred_flag_kernel on arch_filter (the stream); for each SJ-dense / SJ-sparse row its INNER TWIN --
the same inputs as an Inner join under a projection that names only bid columns: the same rows, because a_id is unique on the right, through code the
Semi / Anti paths do not touch.  Row counts are checked against numpy's isin over the same columns.

Workloads:
  SJ-dense / AJ-dense     bid [anti] semi join (auction WHERE category = c) ON auction = a_id
  SJ-sparse / AJ-sparse   the same with both id columns scrambled (id * 2654435761 mod 2^32, bench.py's join_sparse): no dense range covers them
  SJ-utf8                 auction semi join (auction WHERE category = c) ON item_name = item_name   (a Utf8 key: reported only)
  SJ-small-left           auction semi join bid ON a_id = auction   (6e6 left rows against 9.2e7 right rows: the build-heavy direction; no twin --
                          bids repeat their auction, an Inner join there returns pairs)
  SJ-tiny                 the first 60000 bids semi join the first 3000 auctions, and its inner twin (the inner join's one-workgroup sizes)
"""
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


def field(name, dt):
    return {"data_type": dt, "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": False}


BID = [field("auction", "Int32"), field("bidder", "Int32"), field("price", "Int32"), field("b_date_time", TS)]
AUC = [field("a_id", "Int32"), field("item_name", "Utf8"), field("seller", "Int32"), field("category", "Int32")]
AUC2 = [field(f["name"] + "_2", f["data_type"]) for f in AUC]    # (the right side of SJ-utf8: a second relation of the same columns)


def col(fields, name):
    return {"physical_expr": "column", "name": name, "index": [f["name"] for f in fields].index(name)}


def scan(fields):
    return {"execution_plan": "memory_exec", "schema": {"fields": fields, "metadata": {}}, "projection": list(range(len(fields)))}


def category_is(fields, name, c):
    pred = {"physical_expr": "binary_expr", "op": "Eq", "left": {"physical_expr": "cast_expr", "expr": col(fields, name), "cast_type": "Int64"},
            "right": {"physical_expr": "literal", "value": {"Int64": int(c)}}}
    return {"execution_plan": "filter_exec", "predicate": pred, "input": scan(fields)}


def join(jt, left, lfields, right, rfields, lkey, rkey):
    out = lfields + (rfields if jt == "Inner" else [])
    return {"execution_plan": "hash_join_exec", "left": left, "right": right, "join_type": jt, "mode": "CollectLeft",
            "on": [[col(lfields, lkey), col(rfields, rkey)]], "schema": {"fields": out, "metadata": {}}}


def project_left(plan, lfields):
    return {"execution_plan": "projection_exec", "expr": [[col(lfields, f["name"]), f["name"]] for f in lfields], "input": plan,
            "schema": {"fields": lfields, "metadata": {}}}


PROBES = ("semi_probe_bitmap_flag_kernel", "semi_probe_set_flag_kernel", "semi_ids_flag_kernel", "semi_tiny_kernel", "join_probe_unique_flag_kernel", "join_hash_probe_flag_kernel",
          "join_tiny_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semi_join", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    from flock_amd import GpuContext, NEXMarkSource, Window
    from flock_amd.runtime import ExecutionContext

    gpu = GpuContext(0)
    rng = np.random.default_rng(11)
    g = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid", "auction"), auction_times=True)
    b, au = g.bids, g.auctions
    bid_rb = pa.record_batch([pa.array(b.auction.cpu().numpy()), pa.array(b.bidder.cpu().numpy()), pa.array(b.price.cpu().numpy()),
                              pa.array(b.b_date_time.cpu().numpy()).cast(pa.timestamp("ms"))], names=[f["name"] for f in BID])

    def words(n, lo, hi):
        lens = rng.integers(lo, hi + 1, n).astype(np.int32)
        off = np.zeros(n + 1, np.int32)
        np.cumsum(lens, out=off[1:])
        data = rng.integers(97, 123, int(off[-1]), dtype=np.uint8)
        return pa.StringArray.from_buffers(n, pa.py_buffer(off.tobytes()), pa.py_buffer(data.tobytes()))
    auc_rb = pa.record_batch([pa.array(au.a_id.cpu().numpy()), words(au.rows, 8, 19), pa.array(au.seller.cpu().numpy()), pa.array(au.category.cpu().numpy())],
                             names=[f["name"] for f in AUC])
    del g, b, au
    n_bids, n_auc = bid_rb.num_rows, auc_rb.num_rows
    bid_key, a_id, cat = bid_rb.column("auction").to_numpy(), auc_rb.column("a_id").to_numpy(), auc_rb.column("category").to_numpy()
    cats, counts = np.unique(cat, return_counts=True)
    c = int(cats[np.argmax(counts)])
    in_set = np.isin(bid_key, a_id[cat == c])
    semi_rows, anti_rows = int(in_set.sum()), int(n_bids - in_set.sum())

    def scrambled(rb, name):
        k = (rb.column(name).to_numpy().astype(np.uint32) * np.uint32(2654435761)).view(np.int32)
        return rb.set_column(rb.schema.get_field_index(name), name, pa.array(k))
    sparse_bids, sparse_aucs = scrambled(bid_rb, "auction"), scrambled(auc_rb, "a_id")
    auc2_rb = pa.record_batch([auc_rb.column(i) for i in range(auc_rb.num_columns)], names=[f["name"] for f in AUC2])
    import pyarrow.compute as pc
    utf8_rows = pc.sum(pc.is_in(auc_rb.column("item_name"), value_set=auc_rb.column("item_name").filter(pa.array(cat == c)))).as_py()
    small_left_rows = int(np.isin(a_id, bid_key).sum())

    tiny_bids, tiny_aucs = bid_rb.slice(0, 60_000), auc_rb.slice(0, 3_000)
    tiny_rows = int(np.isin(bid_key[:60_000], a_id[:3_000]).sum())
    out = {"input": {"bids": n_bids, "auctions": n_auc, "category": c, "auctions_in_category": int((cat == c).sum()), "seconds": a.seconds, "eps": a.eps},
           "executes": a.executes,
           "recipe": "plan once, feed once, one untimed execute, then timed executes with the result retained in HBM; kernel times from the library's dispatch-bound "
                     "events over two further executes (the kernel-trace CSV beside this file has rocprofv3's)"}

    def timed(plan, feed, generic_only=False):
        ctx = ExecutionContext([plan], gpu=gpu, generic_only=generic_only)
        try:
            ctx.feed_data_sources(feed)
            pl = ctx.plans[0]
            rows = pl.execute_retain()      # (first execute: arena growth, statistics)
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
            for _ in range(2):
                pl.execute_retain()
            gpu.synchronize()
            stats = gpu.profile_read()
            gpu.profile(False)
        finally:
            ctx.close()
        return int(rows), times, stats

    def entry(rows, times, stats, n_left):
        e = {"result_rows": rows, "ms_min": round(min(times), 4), "ms_median": round(statistics.median(times), 4), "ms_max": round(max(times), 4),
             "ms_all": [round(t, 4) for t in times], "launches_per_execute": sum(v["launches"] for v in stats.values()) / 2,
             "kernels_ms_per_execute": {k: round(v["total_ms"] / 2, 4) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])[:10]},
             "kernel_ms_total_per_execute": round(sum(v["total_ms"] for v in stats.values()) / 2, 4)}
        for k in PROBES:
            st = stats.get(k)
            if st and st["launches"]:
                ms = st["total_ms"] / 2
                alg = 4.0 * n_left + 4.0 * n_left / 32
                e["probe"] = {"kernel": k, "ms_per_execute": round(ms, 4), "algorithmic_bytes": int(alg), "GB_per_s": round(alg / (ms * 1e-3) / 1e9, 1),
                              "frac_of_hbm_peak": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
                break
        return e

    if not a.only:
        plan = json.load(open(os.path.join(ROOT, "tests", "golden", "plans", "arch_filter.json")))
        _, _, stats = timed(plan, [[[bid_rb]]], generic_only=True)
        ms = stats["pred_flag_kernel"]["total_ms"] / stats["pred_flag_kernel"]["launches"]
        alg = 4.0 * n_bids
        out["yardstick_stream"] = {"kernel": "pred_flag_kernel on arch_filter (generic operators)", "bids": n_bids, "ms_per_execute": round(ms, 4),
                                   "algorithmic_bytes": int(alg), "frac_of_hbm_peak": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        print("yardstick", json.dumps(out["yardstick_stream"]), flush=True)

    right = category_is(AUC, "category", c)
    W = [
        ("SJ-dense", join("Semi", scan(BID), BID, right, AUC, "auction", "a_id"), [[[bid_rb]], [[auc_rb]]], semi_rows, n_bids),
        ("SJ-dense-inner-twin", project_left(join("Inner", scan(BID), BID, right, AUC, "auction", "a_id"), BID), [[[bid_rb]], [[auc_rb]]], semi_rows, n_bids),
        ("AJ-dense", join("Anti", scan(BID), BID, right, AUC, "auction", "a_id"), [[[bid_rb]], [[auc_rb]]], anti_rows, n_bids),
        ("SJ-sparse", join("Semi", scan(BID), BID, right, AUC, "auction", "a_id"), [[[sparse_bids]], [[sparse_aucs]]], semi_rows, n_bids),
        ("SJ-sparse-inner-twin", project_left(join("Inner", scan(BID), BID, right, AUC, "auction", "a_id"), BID), [[[sparse_bids]], [[sparse_aucs]]], semi_rows, n_bids),
        ("AJ-sparse", join("Anti", scan(BID), BID, right, AUC, "auction", "a_id"), [[[sparse_bids]], [[sparse_aucs]]], anti_rows, n_bids),
        ("SJ-utf8", join("Semi", scan(AUC), AUC, category_is(AUC2, "category_2", c), AUC2, "item_name", "item_name_2"), [[[auc_rb]], [[auc2_rb]]], utf8_rows, n_auc),
        ("SJ-small-left", join("Semi", scan(AUC), AUC, scan(BID), BID, "a_id", "auction"), [[[auc_rb]], [[bid_rb]]], small_left_rows, n_auc),
        # both sides inside the sizes the inner join answers with ONE workgroup (relops.hpp join_is_tiny): semi_tiny_kernel against join_tiny_kernel
        ("SJ-tiny", join("Semi", scan(BID), BID, scan(AUC), AUC, "auction", "a_id"), [[[tiny_bids]], [[tiny_aucs]]], tiny_rows, tiny_bids.num_rows),
        ("SJ-tiny-inner-twin", project_left(join("Inner", scan(BID), BID, scan(AUC), AUC, "auction", "a_id"), BID), [[[tiny_bids]], [[tiny_aucs]]], tiny_rows, tiny_bids.num_rows),
    ]
    for name, plan, feed, want, n_left in W:
        if a.only and name not in a.only.split(","):
            continue
        try:
            rows, times, stats = timed(plan, feed)
            if rows != want:
                raise RuntimeError(f"{name}: {rows} rows, numpy counts {want}")
            e = entry(rows, times, stats, n_left)
        except Exception as ex:   # (a workload that fails is reported, the others still run)
            e = {"error": repr(ex)}
        out[name] = e
        print(name, json.dumps(e), flush=True)
    y = out.get("yardstick_stream", {}).get("frac_of_hbm_peak")
    for name in ("SJ-dense", "AJ-dense", "SJ-sparse", "AJ-sparse"):
        if y and "probe" in out.get(name, {}):
            out[name]["probe"]["over_stream_yardstick"] = round(out[name]["probe"]["frac_of_hbm_peak"] / y, 3)
    for name in ("SJ-dense", "SJ-sparse", "SJ-tiny"):
        s, t = out.get(name, {}), out.get(name + "-inner-twin", {})
        if "ms_median" in s and "ms_median" in t:
            out[name]["vs_inner_twin"] = {"median_ratio": round(s["ms_median"] / t["ms_median"], 3), "twin_spread_ms": round(t["ms_max"] - t["ms_min"], 4),
                                          "no_slower_within_twin_spread": bool(s["ms_median"] <= t["ms_median"] + (t["ms_max"] - t["ms_min"])),
                                          "probe_ms": s.get("probe", {}).get("ms_per_execute"), "twin_probe_ms": t.get("probe", {}).get("ms_per_execute")}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else v.get("ms_median", v.get("ms_per_execute", v.get("error")))) for k, v in out.items() if k != "input"}))
    gpu.close()
    if any(isinstance(v, dict) and "error" in v for v in out.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
