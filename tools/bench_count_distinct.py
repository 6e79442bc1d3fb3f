"""COUNT(DISTINCT x) (distinct.hpp) on the inputs of bench.py's arch_ops: 100 s of NEXMark events at 1e6 events/s -- 9.2e7 bids.  Each statement is planned once,
fed once, executed once untimed (its result checked against numpy) and 10 times timed with its result kept in HBM (flockgpu_plan_execute_retain); reported per
statement: min / median / max ms per execute, kernel launches per execute, the kernels' times from the library's dispatch-bound events, and for the insert
kernel its algorithmic bytes (4 per Int32 argument, 4 more per group id) against the 8 TB/s HBM peak.  Writes profiles/count_distinct/bench.json (or --out).

Statements:
  CD-grouped     SELECT auction, COUNT(*), COUNT(DISTINCT bidder) FROM bid GROUP BY auction
  CD-ungrouped   SELECT COUNT(DISTINCT bidder), COUNT(DISTINCT auction) FROM bid
  CD-two-level   the planner's rewrite of a lone distinct count, which executed before this aggregate did -- the yardstick:
                 SELECT auction, COUNT(bidder) FROM (SELECT auction, bidder FROM bid GROUP BY auction, bidder) GROUP BY auction
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


def field(name, dt, nullable=False):
    return {"data_type": dt, "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


BID = [field("auction", "Int32"), field("bidder", "Int32"), field("price", "Int32"), field("b_date_time", TS)]


def col(fields, name):
    return {"physical_expr": "column", "name": name, "index": [f["name"] for f in fields].index(name)}


def scan(fields):
    return {"execution_plan": "memory_exec", "schema": {"fields": fields, "metadata": {}}, "projection": list(range(len(fields)))}


def count(arg, fields):
    e = col(fields, arg) if arg else {"physical_expr": "literal", "value": {"UInt8": 1}}
    return {"aggregate_expr": "count", "name": "COUNT(%s)" % (arg or "UInt8(1)"), "data_type": "UInt64", "nullable": True, "expr": e}


def distinct(arg, fields):
    return {"aggregate_expr": "distinct_count", "name": "COUNT(DISTINCT %s)" % arg, "data_type": "UInt64", "nullable": True, "exprs": [col(fields, arg)],
            "state_data_types": ["Int32"], "input_data_types": ["Int32"]}


def statement(keys, entries, inp, fields):
    """Partial -> (Hash repartition | CoalescePartitions) -> Final*, as the planner writes it; the nodes' own schemas are not read"""
    def node(mode, group, below):
        return {"execution_plan": "hash_aggregate_exec", "mode": mode, "group_expr": group, "aggr_expr": entries, "input": below,
                "input_schema": {"fields": fields, "metadata": {}}, "schema": {"fields": [], "metadata": {}}}
    part = node("Partial", [[col(fields, k), k] for k in keys], inp)
    pos = [{"physical_expr": "column", "name": k, "index": i} for i, k in enumerate(keys)]
    if not keys:
        return node("Final", [], {"execution_plan": "coalesce_partitions_exec", "input": part})
    return node("FinalPartitioned", [[p, k] for p, k in zip(pos, keys)], {"execution_plan": "repartition_exec", "input": part, "partitioning": {"Hash": [pos, 8]}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count_distinct", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    from flock_amd import GpuContext, NEXMarkSource, Window
    from flock_amd.runtime import ExecutionContext

    gpu = GpuContext(0)
    g = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid",))
    b = g.bids
    auction, bidder = b.auction.cpu().numpy(), b.bidder.cpu().numpy()
    bid_rb = pa.record_batch([pa.array(auction), pa.array(bidder), pa.array(b.price.cpu().numpy()), pa.array(b.b_date_time.cpu().numpy()).cast(pa.timestamp("ms"))],
                             names=[f["name"] for f in BID])
    del g, b
    n = bid_rb.num_rows
    t0 = time.perf_counter()
    pairs = np.unique((auction.astype(np.int64) << 32) | bidder.astype(np.int64).astype(np.uint32))
    per_auction = dict(zip(*[x.tolist() for x in np.unique(pairs >> 32, return_counts=True)]))
    rows_per_auction = dict(zip(*[x.tolist() for x in np.unique(auction, return_counts=True)]))
    n_bidders, n_auctions = len(np.unique(bidder)), len(per_auction)
    cpu_ms = round((time.perf_counter() - t0) * 1e3, 1)
    out = {"input": {"bids": n, "auctions": n_auctions, "bidders": n_bidders, "distinct_pairs": int(len(pairs)), "seconds": a.seconds, "eps": a.eps}, "executes": a.executes,
           "cpu_reference_ms": cpu_ms,
           "recipe": "plan once, feed once, one untimed execute (checked against numpy), then timed executes with the result retained in HBM; kernel times from the "
                     "library's dispatch-bound events over two further executes"}

    def rows_of(rb):
        return sorted(zip(*[rb.column(i).to_pylist() for i in range(rb.num_columns)]))

    def timed(plan, check):
        ctx = ExecutionContext([plan], gpu=gpu)
        try:
            ctx.feed_data_sources([[[bid_rb]]])
            first = ctx.execute()[0][0]     # (first execute: arena growth, the table sized for two slots per row; its rows are checked)
            check(rows_of(first))
            pl = ctx.plans[0]
            gpu.synchronize()
            times = []
            for _ in range(a.executes):
                t0 = time.perf_counter()
                pl.execute_retain()
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
        return times, stats

    def entry(times, stats, insert_bytes):
        e = {"ms_min": round(min(times), 4), "ms_median": round(statistics.median(times), 4), "ms_max": round(max(times), 4), "ms_all": [round(t, 4) for t in times],
             "launches_per_execute": sum(v["launches"] for v in stats.values()) / 2,
             "kernels_ms_per_execute": {k: round(v["total_ms"] / 2, 4) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])[:12]},
             "kernel_ms_total_per_execute": round(sum(v["total_ms"] for v in stats.values()) / 2, 4)}
        st = stats.get("distinct_insert_kernel")
        if st and st["launches"] and insert_bytes:
            ms = st["total_ms"] / 2
            e["insert"] = {"launches_per_execute": st["launches"] / 2, "ms_per_execute": round(ms, 4), "algorithmic_bytes": int(insert_bytes),
                           "GB_per_s": round(insert_bytes / (ms * 1e-3) / 1e9, 1), "frac_of_hbm_peak": round(insert_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        return e

    def same(want):
        def check(got):
            if got != want:
                raise RuntimeError("%d rows, first %s; numpy has %d rows, first %s" % (len(got), got[:2], len(want), want[:2]))
        return check

    grouped_want = sorted((k, rows_per_auction[k], per_auction[k]) for k in per_auction)
    pair_fields = [field("auction", "Int32", True), field("bidder", "Int32", True)]
    inner = statement(["auction", "bidder"], [], scan(BID), BID)
    W = [
        ("CD-grouped", statement(["auction"], [count(None, BID), distinct("bidder", BID)], scan(BID), BID), same(grouped_want), 8.0 * n),
        ("CD-ungrouped", statement([], [distinct("bidder", BID), distinct("auction", BID)], scan(BID), BID), same([(n_bidders, n_auctions)]), 2 * 4.0 * n),
        ("CD-two-level", statement(["auction"], [count("bidder", pair_fields)], inner, pair_fields), same([(k, c) for k, _, c in grouped_want]), 0),
    ]
    for name, plan, check, insert_bytes in W:
        try:
            e = entry(*timed(plan, check), insert_bytes)
        except Exception as ex:   # (a statement that fails is reported, the others still run)
            e = {"error": repr(ex)}
        out[name] = e
        print(name, json.dumps(e), flush=True)
    g_, t_ = out.get("CD-grouped", {}), out.get("CD-two-level", {})
    if "ms_median" in g_ and "ms_median" in t_:
        out["grouped_vs_two_level"] = {"ms_median": g_["ms_median"], "two_level_ms_median": t_["ms_median"], "two_level_spread_ms": round(t_["ms_max"] - t_["ms_min"], 4),
                                       "faster": bool(g_["ms_median"] < t_["ms_median"])}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v.get("ms_median", v.get("error")) if isinstance(v, dict) and k.startswith("CD-") else v for k, v in out.items() if k not in ("input", "recipe")}))
    gpu.close()
    if any(isinstance(v, dict) and "error" in v for v in out.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
