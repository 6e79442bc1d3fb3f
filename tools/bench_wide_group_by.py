"""GROUP BY with five to sixteen accumulators per node (groupwide.hpp) on the inputs of bench.py's arch_ops: 100 s of NEXMark events at 1e6 events/s -- 9.2e7 bids.
Each statement is planned once, fed once, executed once untimed (its totals checked against numpy) and 10 times timed with its result kept in HBM
(flockgpu_plan_execute_retain); reported per statement: min / median / max ms per execute, kernel launches per execute, the kernels' times from the library's
dispatch-bound events, and for the wide pass its algorithmic bytes (the group ids, every distinct argument and validity column once) against the 8 TB/s HBM peak.
Writes profiles/wide_group_by/bench.json (or --out).

Statements (one Partial node each: the pass over the bids is what is measured):
  W-q17          NEXMark q17 as ONE node: COUNT(*), three COUNT(CASE WHEN price ... THEN 1 END), MIN / MAX / AVG / SUM(price) GROUP BY auction, day -- nine accumulators
  W-16-one       sixteen accumulators over price alone
  W-16-eight     sixteen accumulators over eight columns (the bid's four and four computed from them)
  G-4            four accumulators GROUP BY auction: the path this feature must not move (the same kernel names before and after)
--split (runs at the commit before the feature too; the yardstick): q17 as the three GROUP BY plans of at most four accumulators a user had to write --
  S-1 COUNT(*) + the three conditional counts, S-2 MIN / MAX / SUM(price), S-3 AVG(price) -- and the SUM of their executes, beside G-4.
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
WIDE_KERNELS = ("wide_group_init_kernel", "wide_group_kernel", "wide_group_finish_kernel")


def field(name, dt, nullable=False):
    return {"data_type": dt, "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


BID = [field("auction", "Int32"), field("bidder", "Int32"), field("price", "Int32"), field("b_date_time", TS)]


def col(name):
    return {"physical_expr": "column", "name": name, "index": [f["name"] for f in BID].index(name)}


def lit(ty, v):
    return {"physical_expr": "literal", "value": {ty: v}}


def binary(l, op, r):
    return {"physical_expr": "binary_expr", "left": l, "op": op, "right": r}


def agg(fn, name, ty, expr):
    return {"aggregate_expr": fn, "name": name, "data_type": ty, "nullable": True, "expr": expr}


def rank(name, pred):
    case = {"physical_expr": "case_expr", "expr": None, "when_then_expr": [[pred, lit("Int64", 1)]], "else_expr": None}
    return agg("count", name, "UInt64", case)


PRICE = col("price")
DAY = {"physical_expr": "scalar_function_expr", "name": "date_trunc", "args": [lit("Utf8", "day"), col("b_date_time")], "return_type": TS}
COUNTS = [agg("count", "total_bids", "UInt64", lit("UInt8", 1)), rank("rank1_bids", binary(PRICE, "Lt", lit("Int32", 10000))),
          rank("rank2_bids", binary(binary(PRICE, "GtEq", lit("Int32", 10000)), "And", binary(PRICE, "Lt", lit("Int32", 1000000)))),
          rank("rank3_bids", binary(PRICE, "GtEq", lit("Int32", 1000000)))]
EXTREMES = [agg("min", "MIN(price)", "Int32", PRICE), agg("max", "MAX(price)", "Int32", PRICE), agg("sum", "SUM(price)", "Int64", PRICE)]
AVG = [agg("avg", "AVG(price)", "Float64", PRICE)]
Q17_KEYS = [[col("auction"), "auction"], [DAY, "day"]]


def partial(group, entries):
    """one Partial node over the bids (the node's own schema is not read)"""
    return {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": group, "aggr_expr": entries,
            "input": {"execution_plan": "memory_exec", "schema": {"fields": BID, "metadata": {"name": "bid"}}, "projection": [0, 1, 2, 3]},
            "input_schema": {"fields": BID, "metadata": {}}, "schema": {"fields": [], "metadata": {}}}


def sixteen(exprs):
    """sixteen accumulators over the expressions: MIN and MAX of each in turn, (type, expression) pairs"""
    out = []
    for k in range(16):
        ty, e = exprs[(k // 2) % len(exprs)]
        fn = ("min", "max")[k % 2] if len(exprs) > 1 else ("min", "max", "sum", "count")[k % 4]
        out.append(agg(fn, "%s_%d" % (fn, k), "UInt64" if fn == "count" else "Int64" if fn == "sum" else ty, e))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--split", action="store_true", help="q17 as three plans of at most four accumulators each (runs before the feature too)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out_path = a.out or os.path.join(ROOT, "profiles", "wide_group_by", "split.json" if a.split else "bench.json")
    import numpy as np
    import pyarrow as pa
    import pyarrow.compute as pc
    from flock_amd import GpuContext, NEXMarkSource, Window
    from flock_amd.runtime import ExecutionContext

    gpu = GpuContext(0)
    g = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid",))
    b = g.bids
    price = b.price.cpu().numpy()
    bid_rb = pa.record_batch([pa.array(b.auction.cpu().numpy()), pa.array(b.bidder.cpu().numpy()), pa.array(price), pa.array(b.b_date_time.cpu().numpy()).cast(pa.timestamp("ms"))],
                             names=[f["name"] for f in BID])
    del g, b
    n = bid_rb.num_rows
    totals = {"total_bids[count]": n, "rank1_bids[count]": int((price < 10000).sum()), "rank2_bids[count]": int(((price >= 10000) & (price < 1000000)).sum()),
              "rank3_bids[count]": int((price >= 1000000).sum()), "SUM(price)[sum]": int(price.astype(np.int64).sum()), "AVG(price)[count]": n,
              "AVG(price)[sum]": float(price.astype(np.int64).sum())}
    extremes = {"MIN(price)[min]": int(price.min()), "MAX(price)[max]": int(price.max())}
    out = {"input": {"bids": n, "seconds": a.seconds, "eps": a.eps}, "executes": a.executes, "split": a.split,
           "recipe": "plan once, feed once, one untimed execute (column totals checked against numpy), then timed executes with the result retained in HBM; kernel times "
                     "from the library's dispatch-bound events over two further executes"}

    def check(rb):
        """the state columns this tool knows: their sums over the groups (minimum / maximum of the extremes) against numpy"""
        for name in rb.schema.names:
            c = rb.column(rb.schema.names.index(name))
            if name in totals:
                got = pc.sum(c).as_py()
                if got != totals[name]:
                    raise RuntimeError("%s: %r over the groups, numpy has %r" % (name, got, totals[name]))
            elif name in extremes:
                got = (pc.min(c) if "min" in name else pc.max(c)).as_py()
                if got != extremes[name]:
                    raise RuntimeError("%s: %r over the groups, numpy has %r" % (name, got, extremes[name]))
        return rb.num_rows

    def timed(plan):
        ctx = ExecutionContext([plan], gpu=gpu)
        try:
            ctx.feed_data_sources([[[bid_rb]]])
            groups = check(ctx.execute()[0][0])     # (first execute: arena growth; its totals are checked)
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
        return groups, times, stats

    def entry(groups, times, stats, pass_bytes):
        e = {"groups": groups, "ms_min": round(min(times), 4), "ms_median": round(statistics.median(times), 4), "ms_max": round(max(times), 4), "ms_all": [round(t, 4) for t in times],
             "launches_per_execute": sum(v["launches"] for v in stats.values()) / 2,
             "kernels_ms_per_execute": {k: round(v["total_ms"] / 2, 4) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])[:14]},
             "kernel_ms_total_per_execute": round(sum(v["total_ms"] for v in stats.values()) / 2, 4)}
        st = stats.get("wide_group_kernel")
        if st and st["launches"] and pass_bytes:
            ms = st["total_ms"] / 2
            e["wide_pass"] = {"launches_per_execute": st["launches"] / 2, "ms_per_execute": round(ms, 4), "algorithmic_bytes": int(pass_bytes),
                              "GB_per_s": round(pass_bytes / (ms * 1e-3) / 1e9, 1), "frac_of_hbm_peak": round(pass_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                              "init_pass_finish_ms": round(sum(stats[k]["total_ms"] for k in WIDE_KERNELS if k in stats) / 2, 4)}
        return e

    by_auction = [[col("auction"), "auction"]]
    g4 = ("G-4", partial(by_auction, [COUNTS[0]] + EXTREMES), 0)
    if a.split:
        W = [("S-1", partial(Q17_KEYS, COUNTS), 0), ("S-2", partial(Q17_KEYS, EXTREMES), 0), ("S-3", partial(Q17_KEYS, AVG), 0), g4]
    else:
        eight = [("Int32", PRICE), ("Int32", col("bidder")), ("Int32", col("auction")), (TS, col("b_date_time")),
                 ("Int32", binary(PRICE, "Plus", col("bidder"))), ("Int32", binary(col("auction"), "Minus", col("bidder"))),
                 ("Int32", binary(PRICE, "Modulo", lit("Int32", 1000))), ("Int32", binary(col("bidder"), "Multiply", lit("Int32", 3)))]
        # the wide pass's bytes per row: 4 of ids; q17: price 4 and three validity bytes; sixteen over price: 4; over eight columns: 7 x 4 + 8
        W = [("W-q17", partial(Q17_KEYS, COUNTS + EXTREMES[:2] + AVG + EXTREMES[2:]), (4 + 4 + 3) * n), ("W-16-one", partial(by_auction, sixteen([("Int32", PRICE)])), (4 + 4) * n),
             ("W-16-eight", partial(by_auction, sixteen(eight)), (4 + 7 * 4 + 8) * n), g4]
    for name, plan, pass_bytes in W:
        try:
            e = entry(*timed(plan), pass_bytes)
        except Exception as ex:   # (a statement that fails is reported, the others still run)
            e = {"error": repr(ex)}
        out[name] = e
        print(name, json.dumps(e), flush=True)
    if a.split and all("ms_median" in out.get(k, {}) for k in ("S-1", "S-2", "S-3")):
        out["split_sum"] = {"ms_median": round(sum(out[k]["ms_median"] for k in ("S-1", "S-2", "S-3")), 4), "ms_min": round(sum(out[k]["ms_min"] for k in ("S-1", "S-2", "S-3")), 4),
                            "kernel_ms_total_per_execute": round(sum(out[k]["kernel_ms_total_per_execute"] for k in ("S-1", "S-2", "S-3")), 4)}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v.get("ms_median", v.get("error")) for k, v in out.items() if isinstance(v, dict) and ("ms_median" in v or "error" in v)}))
    gpu.close()
    if any(isinstance(v, dict) and "error" in v for v in out.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
