"""CrossJoinExec (cross.hpp) on the inputs of bench.py's arch_ops: 100 s of NEXMark events at 1e6 events/s -- 9.2e7 bids.  Each workload is planned once, fed
once, executed once untimed (its row count checked) and 10 times timed with its result kept in HBM (flockgpu_plan_execute_retain); reported per workload:
mean / min / median / max ms per execute, kernel launches per execute, the kernels' own times (the library's dispatch-bound events, two further executes)
and for the cross-join kernels their bytes -- output bytes written plus source bytes read once -- as a fraction of the 8 TB/s HBM peak.
Writes profiles/cross_join/bench.json (or --out).

Workloads:
  X-avg        SELECT auction, bidder, price, avgp FROM bid CROSS JOIN (SELECT AVG(price) AS avgp FROM bid) a WHERE CAST(price AS Float64) > avgp
               (tests/golden/plans/bids_above_average.json)
  X-avg-key    the same rows through the only route there was before cross_join_exec executed: an inner hash_join_exec on a computed constant key
               (price * 0 = MIN(price) * 0).  This plan runs on either commit: `--baseline-only` at the PARENT commit, handed back with --parent-json
  X-fill       SELECT bid.*, maxp FROM bid CROSS JOIN (SELECT MAX(price) maxp FROM bid): the fill alone, next to textsel's `SELECT 'bid'` fill
  X-small      3e3 x 3e4 rows of (Int32, Int64, Utf8 of ~12 bytes) on both sides: 9e7 output rows, every repeat and tile kernel
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


def schema(fields):
    return {"fields": fields, "metadata": {}}


def col(fields, name):
    return {"physical_expr": "column", "name": name, "index": [f["name"] for f in fields].index(name)}


def lit(ty, v):
    return {"physical_expr": "literal", "value": {ty: v}}


def binary(l, op, r):
    return {"physical_expr": "binary_expr", "left": l, "op": op, "right": r}


def cast(e, ty):
    return {"physical_expr": "cast_expr", "expr": e, "cast_type": ty}


def scan(fields, keep=None):
    return {"execution_plan": "memory_exec", "schema": schema(fields), "projection": list(range(len(fields))) if keep is None else keep}


def project(inp, exprs, fields):
    return {"execution_plan": "projection_exec", "expr": [[e, n] for e, n in exprs], "input": inp, "schema": schema(fields)}


def filt(inp, pred):
    return {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096, "input": {"execution_plan": "filter_exec", "predicate": pred, "input": inp}}


def ungrouped(aggs, inp, in_fields):
    """aggs: [(function, argument column, result type, name)]; Partial -> CoalescePartitions -> Final"""
    entries = [{"aggregate_expr": fn, "name": name, "data_type": ty, "nullable": True, "expr": col(in_fields, arg)} for fn, arg, ty, name in aggs]
    state = []
    for fn, arg, ty, name in aggs:
        state += [field(name + "[count]", "UInt64", True), field(name + "[sum]", "Float64", True)] if fn == "avg" else [field("%s[%s]" % (name, fn), ty, True)]
    part = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": [], "aggr_expr": entries, "input": inp, "input_schema": schema(in_fields),
            "schema": schema(state)}
    return {"execution_plan": "hash_aggregate_exec", "mode": "Final", "group_expr": [], "aggr_expr": entries,
            "input": {"execution_plan": "coalesce_partitions_exec", "input": part}, "input_schema": schema(in_fields),
            "schema": schema([field(name, ty, True) for _, _, ty, name in aggs])}


def cross(left, right, fields):
    return {"execution_plan": "cross_join_exec", "left": left, "right": right, "schema": schema(fields)}


PRICE = [field("price", "Int32")]
THREE = BID[:3]


def x_avg_key():
    """bids above the average through an inner join on a constant key: bid with k = price * 0, the aggregate row with k2 = MIN(price) * 0"""
    lf = THREE + [field("k", "Int32", True)]
    left = project(scan(BID, [0, 1, 2]), [(col(THREE, f["name"]), f["name"]) for f in THREE] + [(binary(col(THREE, "price"), "Multiply", lit("Int32", 0)), "k")], lf)
    af = [field("AVG(bid.price)", "Float64", True), field("MIN(bid.price)", "Int32", True)]
    row = ungrouped([("avg", "price", "Float64", "AVG(bid.price)"), ("min", "price", "Int32", "MIN(bid.price)")], scan(BID, [2]), PRICE)
    rf = [field("avgp", "Float64", True), field("k2", "Int32", True)]
    right = project(row, [(col(af, "AVG(bid.price)"), "avgp"), (binary(col(af, "MIN(bid.price)"), "Multiply", lit("Int32", 0)), "k2")], rf)
    j = {"execution_plan": "hash_join_exec", "left": left, "right": right, "on": [[col(lf, "k"), col(rf, "k2")]], "join_type": "Inner", "mode": "CollectLeft",
         "schema": schema(lf + rf)}
    both = lf + rf
    out = THREE + [field("avgp", "Float64", True)]
    keep = filt(j, binary(cast(col(both, "price"), "Float64"), "Gt", col(both, "avgp")))
    return project(keep, [(col(both, f["name"]), f["name"]) for f in out], out)


def x_fill():
    mx = [field("maxp", "Int32", True)]
    row = project(ungrouped([("max", "price", "Int32", "MAX(bid.price)")], scan(BID, [2]), PRICE), [(col([field("MAX(bid.price)", "Int32")], "MAX(bid.price)"), "maxp")], mx)
    return cross(scan(BID), row, BID + mx)


SMALL_L = [field("a", "Int32"), field("b", "Int64"), field("c", "Utf8")]
SMALL_R = [field("d", "Int32"), field("e", "Int64"), field("f", "Utf8")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--small", default="3000x30000", help="X-small's L x R")
    ap.add_argument("--baseline-only", action="store_true", help="only X-avg-key, the inner join on a constant key (what the parent commit executes)")
    ap.add_argument("--parent-json", default="", help="the --baseline-only output of the parent commit, same session")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_join", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
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
    avg = int(price.sum(dtype=np.int64)) / n
    above = int((price.astype(np.float64) > avg).sum())
    out = {"input": {"bids": n, "bids_above_average": above, "seconds": a.seconds, "eps": a.eps}, "executes": a.executes,
           "recipe": "plan once, feed once, one untimed execute (row count checked against numpy), then timed executes with the result retained in HBM; kernel times "
                     "from the library's dispatch-bound events over two further executes; bytes = output bytes written + source bytes read once"}

    def timed(plan, feed, want_rows):
        ctx = ExecutionContext([plan], gpu=gpu)
        try:
            ctx.feed_data_sources(feed)
            pl = ctx.plans[0]
            rows = pl.execute_retain()          # (first execute: arena growth, statistics)
            if rows != want_rows:
                raise RuntimeError("%d rows, numpy has %d" % (rows, want_rows))
            for _ in range(2):                  # (warm-up: the clocks settle over the first dozen calls -- these, the timed ones run after them)
                pl.execute_retain()
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
            samples = {k: gpu.profile_samples(k) for k in stats if k.startswith("cross_") or k == "textsel_fill_kernel"}
            gpu.profile(False)
        finally:
            ctx.close()
        return times, stats, samples

    def entry(times, stats):
        return {"ms_mean": round(statistics.mean(times), 4), "ms_min": round(min(times), 4), "ms_median": round(statistics.median(times), 4), "ms_max": round(max(times), 4),
                "ms_all": [round(t, 4) for t in times], "launches_per_execute": sum(v["launches"] for v in stats.values()) / 2,
                "kernels_ms_per_execute": {k: round(v["total_ms"] / 2, 4) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])[:12]},
                "kernel_ms_total_per_execute": round(sum(v["total_ms"] for v in stats.values()) / 2, 4)}

    def rate(ms, nbytes):
        return {"ms": round(ms, 4), "bytes": int(nbytes), "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1), "frac_of_hbm_peak": round(nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}

    def run(key, fn):
        try:
            e = fn()
        except Exception as ex:   # (a workload that fails is reported, the others still run)
            e = {"error": repr(ex)}
        out[key] = e
        print(key, json.dumps(e), flush=True)

    feed = [[[bid_rb]]]

    def w_avg_key():
        times, stats, _ = timed(x_avg_key(), feed, above)
        return entry(times, stats)
    run("X-avg-key", w_avg_key)

    if not a.baseline_only:
        def w_avg():
            times, stats, samples = timed(json.load(open(os.path.join(ROOT, "tests", "golden", "plans", "bids_above_average.json"))), feed, above)
            e = entry(times, stats)
            fill = samples.get("cross_fill_kernel", [])
            if fill:   # avgp: 8 bytes per bid written, one value read
                e["fill_avgp"] = rate(statistics.median(fill), 8.0 * n)
            return e
        run("X-avg", w_avg)

        def w_fill():
            times, stats, samples = timed(x_fill(), feed, n)
            e = entry(times, stats)
            fill = samples.get("cross_fill_kernel", [])
            if fill:   # maxp: 4 bytes per bid written; nothing per bid column
                e["fill_maxp"] = rate(statistics.median(fill), 4.0 * n)
            e["cross_kernels"] = sorted(k for k in stats if k.startswith("cross_"))
            return e
        run("X-fill", w_fill)

        def w_textsel_fill():   # the project's own fill reading, in this process: SELECT 'bid' FROM bid (Utf8: 4 bytes of offsets + 3 bytes per row)
            plan = project(scan(BID, [0]), [(lit("Utf8", "bid"), "label")], [field("label", "Utf8", True)])
            times, stats, samples = timed(plan, feed, n)
            e = entry(times, stats)
            s = samples.get("textsel_fill_kernel", [])
            if s:
                e["fill_label"] = rate(statistics.median(s), 7.0 * n)
            return e
        run("textsel-fill", w_textsel_fill)

        def w_small():
            L, R = (int(x) for x in a.small.split("x"))
            r = np.random.default_rng(5)

            def side(rows, names, tag):
                text = ["%s%011d" % (tag, int(x)) for x in r.integers(0, 10**11, rows)]     # 12 bytes each
                return pa.record_batch([pa.array(r.integers(-2**31, 2**31, rows, dtype=np.int64).astype(np.int32)), pa.array(r.integers(-2**62, 2**62, rows, dtype=np.int64)),
                                        pa.array(text)], names=names)
            lrb, rrb = side(L, [f["name"] for f in SMALL_L], "l"), side(R, [f["name"] for f in SMALL_R], "r")
            N = L * R
            times, stats, samples = timed(cross(scan(SMALL_L), scan(SMALL_R), SMALL_L + SMALL_R), [[[lrb]], [[rrb]]], N)
            e = entry(times, stats)
            e["shape"] = {"L": L, "R": R, "rows": N, "utf8_bytes_per_value": 12}
            med = lambda k, i, per: statistics.median(samples[k][i::per]) if len(samples.get(k, [])) >= per else None     # launch i of `per` launches per execute
            parts = {"repeat_int32": ("cross_repeat_kernel", 0, 2, 4.0 * N + 4.0 * L), "repeat_int64": ("cross_repeat_kernel", 1, 2, 8.0 * N + 8.0 * L),
                     "tile_int32": ("cross_tile_kernel", 0, 2, 4.0 * N + 4.0 * R), "tile_int64": ("cross_tile_kernel", 1, 2, 8.0 * N + 8.0 * R),
                     "repeat_offsets": ("cross_offsets_kernel", 0, 2, 4.0 * N + 4.0 * L), "tile_offsets": ("cross_offsets_kernel", 1, 2, 4.0 * N + 4.0 * R),
                     "repeat_bytes": ("cross_repeat_bytes_kernel", 0, 1, 12.0 * N + 12.0 * L + 4.0 * L), "tile_bytes": ("cross_tile_bytes_kernel", 0, 1, 12.0 * N + 12.0 * R)}
            e["kernels"] = {}
            for name, (k, i, per, nbytes) in parts.items():
                ms = med(k, i, per)
                if ms:
                    e["kernels"][name] = rate(ms, nbytes)
            return e
        run("X-small", w_small)

    if a.parent_json:
        parent = json.load(open(a.parent_json))
        out["parent"] = {"X-avg-key": parent.get("X-avg-key")}
        u, p = out.get("X-avg", {}), parent.get("X-avg-key") or {}
        if "ms_mean" in u and "ms_mean" in p:
            spread = p["ms_max"] - p["ms_min"]
            out["X-avg"]["vs_parent_constant_key_join"] = {"parent_ms_mean": p["ms_mean"], "parent_ms_median": p["ms_median"], "parent_spread_ms": round(spread, 4),
                                                           "ms_mean": u["ms_mean"], "ms_median": u["ms_median"], "speedup_of_means": round(p["ms_mean"] / u["ms_mean"], 2),
                                                           "faster_by_more_than_parent_spread": bool(u["ms_median"] < p["ms_median"] - spread)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else v.get("ms_mean", v.get("error"))) for k, v in out.items() if k not in ("input", "parent")}))
    gpu.close()
    if any(isinstance(v, dict) and "error" in v for v in out.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
