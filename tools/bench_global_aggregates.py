"""Ungrouped aggregates (HashAggregateExec without GROUP BY, reduce.hpp) on the inputs of bench.py's arch_ops: 100 s of NEXMark events at 1e6 events/s --
9.2e7 bids.  Each workload is planned once, fed once, executed once untimed and 10 times timed with its result kept in HBM (flockgpu_plan_execute_retain);
reported per workload: min / median / max ms per execute, kernel launches per execute, the kernels' times, and for the reduce kernel its algorithmic bytes
(4 per Int32 value, 8 per 64-bit value, 4 per 32 rows of flag words) as a fraction of the 8 TB/s HBM peak and of the stream yardstick.
Writes profiles/global_aggregates/bench.json (or --out).

Yardstick, measured in the same process: pred_flag_kernel on arch_filter (the stream).  Every row also stands beside what a user could write before
ungrouped aggregates executed: the same statement as `GROUP BY price * 0` (one group, dense_group_kernel; without the AVG where the list has one -- a GROUP BY
node carries four accumulators, and AVG is SUM / COUNT of what stays) -- run with --grouped-only at the PARENT commit
in the same session and handed back with --parent-json; the ungrouped form has to beat the parent's median by more than the parent's own min-max spread.
Results are checked against numpy over the same columns (whose own times are reported as the CPU reference).

Workloads:
  GA-count-filter   COUNT(*) WHERE auction % 123 = 0            (the arch_filter predicate: the predicate pass plus a fold)
  GA-price          COUNT(*), SUM(price), MIN(price), MAX(price), AVG(price)
  GA-filtered       the same WHERE auction % 123 = 0
  GA-two-columns    MAX(b_date_time), SUM(price)
  GA-final          Final over 8 Partial state rows of GA-price (launch-bound)
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
RESULT = {"count": lambda t: "UInt64", "avg": lambda t: "Float64", "sum": lambda t: "Int64", "min": lambda t: t, "max": lambda t: t}


def col(fields, name):
    return {"physical_expr": "column", "name": name, "index": [f["name"] for f in fields].index(name)}


def lit(ty, v):
    return {"physical_expr": "literal", "value": {ty: v}}


def binary(l, op, r):
    return {"physical_expr": "binary_expr", "left": l, "op": op, "right": r}


def scan(fields):
    return {"execution_plan": "memory_exec", "schema": {"fields": fields, "metadata": {}}, "projection": list(range(len(fields)))}


def arch_filter(inp):
    pred = binary(binary({"physical_expr": "cast_expr", "expr": col(BID, "auction"), "cast_type": "Int64"}, "Modulo", lit("Int64", 123)), "Eq", lit("Int64", 0))
    return {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096, "input": {"execution_plan": "filter_exec", "predicate": pred, "input": inp}}


def name_of(fn, arg):
    return "%s(%s)" % (fn.upper(), arg or "UInt8(1)")


def entries(aggs, fields):
    types = {f["name"]: f["data_type"] for f in fields}
    return [{"aggregate_expr": fn, "name": name_of(fn, arg), "data_type": RESULT[fn](types[arg] if arg else None), "nullable": True,
             "expr": col(fields, arg) if arg else lit("UInt8", 1)} for fn, arg in aggs]


def state_fields(aggs, fields):
    types = {f["name"]: f["data_type"] for f in fields}
    out = []
    for fn, arg in aggs:
        n = name_of(fn, arg)
        if fn == "avg":
            out += [field(n + "[count]", "UInt64", True), field(n + "[sum]", "Float64", True)]
        else:
            out.append(field("%s[%s]" % (n, fn), RESULT[fn](types[arg] if arg else None), True))
    return out


def aggregate(mode, aggs, inp, fields, group=None):
    """group: None, or (expression, name, type) -- the GROUP BY twin"""
    ge = [] if group is None else [[group[0], group[1]]]
    key = [] if group is None else [field(group[1], group[2], True)]
    types = {f["name"]: f["data_type"] for f in fields}
    sch = key + (state_fields(aggs, fields) if mode == "Partial" else [field(name_of(fn, arg), RESULT[fn](types[arg] if arg else None), True) for fn, arg in aggs])
    return {"execution_plan": "hash_aggregate_exec", "mode": mode, "group_expr": ge, "aggr_expr": entries(aggs, fields), "input": inp,
            "input_schema": {"fields": fields, "metadata": {}}, "schema": {"fields": sch, "metadata": {}}}


def statement(aggs, inp, grouped):
    """Partial -> (CoalescePartitions | Hash repartition) -> Final, as the planner writes the statement; grouped: ... GROUP BY price * 0"""
    if not grouped:
        return aggregate("Final", aggs, {"execution_plan": "coalesce_partitions_exec", "input": aggregate("Partial", aggs, inp, BID)}, BID)
    g = (binary(col(BID, "price"), "Multiply", lit("Int32", 0)), "g", "Int32")
    part = aggregate("Partial", aggs, inp, BID, g)
    key0 = {"physical_expr": "column", "name": "g", "index": 0}
    rep = {"execution_plan": "repartition_exec", "input": part, "partitioning": {"Hash": [[key0], 4]}}
    return aggregate("FinalPartitioned", aggs, rep, BID, (key0, "g", "Int32"))


PRICE5 = [("count", None), ("sum", "price"), ("min", "price"), ("max", "price"), ("avg", "price")]


def twin(aggs):
    """What the GROUP BY form can carry: four accumulators per node (relops.hpp kMaxGroupAggs) -- the list without its AVG, which is SUM / COUNT of what stays"""
    return [x for x in aggs if x[0] != "avg"]


TWO = [("max", "b_date_time"), ("sum", "price")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--grouped-only", action="store_true", help="only the GROUP BY price * 0 forms (what the parent commit executes)")
    ap.add_argument("--parent-json", default="", help="the --grouped-only output of the parent commit, same session")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_aggregates", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    from flock_amd import GpuContext, NEXMarkSource, Window
    from flock_amd.runtime import ExecutionContext

    gpu = GpuContext(0)
    g = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid",))
    b = g.bids
    auction, price, when = b.auction.cpu().numpy(), b.price.cpu().numpy(), b.b_date_time.cpu().numpy()
    bid_rb = pa.record_batch([pa.array(auction), pa.array(b.bidder.cpu().numpy()), pa.array(price), pa.array(when).cast(pa.timestamp("ms"))], names=[f["name"] for f in BID])
    del g, b
    n = bid_rb.num_rows

    def cpu(fn):
        t0 = time.perf_counter()
        v = fn()
        return v, round((time.perf_counter() - t0) * 1e3, 2)
    keep, keep_ms = cpu(lambda: auction.astype(np.int64) % 123 == 0)

    def five(p):
        s = int(p.sum(dtype=np.int64))
        return [len(p), s, int(p.min()), int(p.max()), s / len(p)]
    want, cpu_ms = {}, {}
    want["GA-count-filter"], cpu_ms["GA-count-filter"] = [int(keep.sum())], keep_ms
    want["GA-price"], cpu_ms["GA-price"] = cpu(lambda: five(price))
    want["GA-filtered"], cpu_ms["GA-filtered"] = cpu(lambda: five(price[keep]))
    cpu_ms["GA-filtered"] += keep_ms
    want["GA-two-columns"], cpu_ms["GA-two-columns"] = cpu(lambda: [int(when.max()), int(price.sum(dtype=np.int64))])
    want["GA-final"] = want["GA-price"]
    # GA-final: eight Partial state rows of GA-price, computed here
    cuts = [n * k // 8 for k in range(9)]
    rows8 = [five(price[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])]
    sf = state_fields(PRICE5, BID)
    cols8 = [[r[0] for r in rows8], [r[1] for r in rows8], [r[2] for r in rows8], [r[3] for r in rows8], [r[0] for r in rows8], [float(r[1]) for r in rows8]]
    pa_t = {"UInt64": pa.uint64(), "Int64": pa.int64(), "Int32": pa.int32(), "Float64": pa.float64()}
    state_rb = pa.record_batch([pa.array(c, pa_t[f["data_type"]]) for c, f in zip(cols8, sf)], names=[f["name"] for f in sf])
    gkey = field("g", "Int32", True)
    state_rb_g = pa.record_batch([pa.array([0] * 8, pa.int32())] + [state_rb.column(i) for i in range(state_rb.num_columns)], names=["g"] + state_rb.schema.names)
    key0 = {"physical_expr": "column", "name": "g", "index": 0}
    final_plain = aggregate("Final", PRICE5, scan(sf), BID)
    sf4 = state_fields(twin(PRICE5), BID)
    state_rb_g = pa.record_batch([state_rb_g.column(i) for i in range(1 + len(sf4))], names=state_rb_g.schema.names[:1 + len(sf4)])
    final_grouped = aggregate("FinalPartitioned", twin(PRICE5), scan([gkey] + sf4), BID, (key0, "g", "Int32"))

    out = {"input": {"bids": n, "kept_by_filter": int(keep.sum()), "seconds": a.seconds, "eps": a.eps}, "executes": a.executes,
           "recipe": "plan once, feed once, one untimed execute (checked against numpy), then timed executes with the result retained in HBM; kernel times from the "
                     "library's dispatch-bound events over two further executes", "cpu_reference_ms": cpu_ms}

    def row_of(rb):
        return [rb.column(i).cast(pa.int64()).to_pylist()[0] if pa.types.is_timestamp(rb.column(i).type) else rb.column(i).to_pylist()[0] for i in range(rb.num_columns)]

    def timed(plan, feed, generic_only=False, check=None, skip=0):
        ctx = ExecutionContext([plan], gpu=gpu, generic_only=generic_only)
        try:
            ctx.feed_data_sources(feed)
            first = ctx.execute()[0][0]     # (first execute: arena growth, statistics; its row is checked)
            if check is not None and (first.num_rows != 1 or row_of(first)[skip:] != check):
                raise RuntimeError("%s rows, %s; numpy has %s" % (first.num_rows, row_of(first)[skip:] if first.num_rows == 1 else "-", check))
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

    def entry(times, stats, alg_bytes):
        e = {"ms_min": round(min(times), 4), "ms_median": round(statistics.median(times), 4), "ms_max": round(max(times), 4),
             "ms_all": [round(t, 4) for t in times], "launches_per_execute": sum(v["launches"] for v in stats.values()) / 2,
             "kernels_ms_per_execute": {k: round(v["total_ms"] / 2, 4) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])[:10]},
             "kernel_ms_total_per_execute": round(sum(v["total_ms"] for v in stats.values()) / 2, 4)}
        st = stats.get("global_reduce_kernel")
        if st and st["launches"] and alg_bytes:
            ms = st["total_ms"] / 2
            e["reduce"] = {"ms_per_execute": round(ms, 4), "algorithmic_bytes": int(alg_bytes), "GB_per_s": round(alg_bytes / (ms * 1e-3) / 1e9, 1),
                           "frac_of_hbm_peak": round(alg_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        return e

    if not a.grouped_only:
        plan = json.load(open(os.path.join(ROOT, "tests", "golden", "plans", "arch_filter.json")))
        _, stats = timed(plan, [[[bid_rb]]], generic_only=True)
        ms = stats["pred_flag_kernel"]["total_ms"] / stats["pred_flag_kernel"]["launches"]
        out["yardstick_stream"] = {"kernel": "pred_flag_kernel on arch_filter (generic operators)", "bids": n, "ms_per_execute": round(ms, 4),
                                   "algorithmic_bytes": int(4.0 * n), "frac_of_hbm_peak": round(4.0 * n / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        print("yardstick", json.dumps(out["yardstick_stream"]), flush=True)

    feed = [[[bid_rb]]]
    W = [
        ("GA-count-filter", [("count", None)], arch_filter, feed, 0),
        ("GA-price", PRICE5, lambda x: x, feed, 4.0 * n),
        ("GA-filtered", PRICE5, arch_filter, feed, 4.0 * n + 4.0 * n / 32),
        ("GA-two-columns", TWO, lambda x: x, feed, 12.0 * n),
    ]
    for name, aggs, over, fd, alg in W:
        for grouped in ([True] if a.grouped_only else [False, True]):
            key = name + ("-grouped" if grouped else "")
            try:
                use = twin(aggs) if grouped else aggs
                times, stats = timed(statement(use, over(scan(BID)), grouped), fd, check=want[name][:len(use)], skip=1 if grouped else 0)
                e = entry(times, stats, alg)
            except Exception as ex:   # (a workload that fails is reported, the others still run)
                e = {"error": repr(ex)}
            out[key] = e
            print(key, json.dumps(e), flush=True)
    for grouped in ([True] if a.grouped_only else [False, True]):
        key = "GA-final" + ("-grouped" if grouped else "")
        try:
            times, stats = timed(final_grouped if grouped else final_plain, [[[state_rb_g if grouped else state_rb]]],
                                 check=want["GA-final"][:len(twin(PRICE5)) if grouped else None], skip=1 if grouped else 0)
            e = entry(times, stats, 0)
        except Exception as ex:
            e = {"error": repr(ex)}
        out[key] = e
        print(key, json.dumps(e), flush=True)

    y = out.get("yardstick_stream", {}).get("frac_of_hbm_peak")
    for name in ("GA-price", "GA-filtered", "GA-two-columns"):
        if y and "reduce" in out.get(name, {}):
            out[name]["reduce"]["over_stream_yardstick"] = round(out[name]["reduce"]["frac_of_hbm_peak"] / y, 3)
    if a.parent_json:
        parent = json.load(open(a.parent_json))
        out["parent_grouped"] = {k: v for k, v in parent.items() if k.endswith("-grouped")}
        for name in ("GA-count-filter", "GA-price", "GA-filtered", "GA-two-columns", "GA-final"):
            u, p = out.get(name, {}), parent.get(name + "-grouped", {})
            if "ms_median" in u and "ms_median" in p:
                spread = p["ms_max"] - p["ms_min"]
                out[name]["vs_parent_group_by"] = {"parent_ms_median": p["ms_median"], "parent_spread_ms": round(spread, 4), "ms_median": u["ms_median"],
                                                   "faster_by_more_than_parent_spread": bool(u["ms_median"] < p["ms_median"] - spread)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else v.get("ms_median", v.get("ms_per_execute", v.get("error")))) for k, v in out.items() if k not in ("input", "parent_grouped")}))
    gpu.close()
    if any(isinstance(v, dict) and "error" in v for v in out.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
