"""UnionExec (union.hpp) on the inputs of bench.py's arch_ops: 100 s of NEXMark events at 1e6 events/s -- 9.2e7 bids.  Each workload is planned once, fed once,
executed once untimed (its row count checked against numpy) and --executes times timed; kernel times come from the library's dispatch-bound events over two
further executes.  Writes profiles/union/bench.json (or --out).

Workloads:
  U-two-ranges   tests/golden/plans/bids_two_ranges.json: two filters of ONE fed `bid` source that read different columns of it, results to the host (the
                 second filter's instant is set to the median b_date_time of the generated bids)
  U-activity     tests/golden/plans/person_activity.json: the event log over auction (one row per 46 bids, made here) and bid under GROUP BY person, kind
  U-copy         bid UNION ALL bid of (Int32, Int32, Int32, Timestamp, Utf8 of 12 bytes) over the first --copy-rows bids, result retained in HBM: the fixed,
                 offsets and bytes kernels, their bytes -- output written plus source read once -- as fractions of the 8 TB/s HBM peak
  *-separate     the only route there was before union_exec executed: every branch as a plan of its own, each result brought to the host and the results
                 appended there (pyarrow.concat_tables).  These plans run on either commit: `--baseline-only` at the PARENT commit.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PLANS = os.path.join(ROOT, "tests", "golden", "plans")
HBM_PEAK_GBS = 8000.0
TS = {"Timestamp": ["Millisecond", None]}


def field(name, dt, nullable=False):
    return {"data_type": dt, "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


BID5 = [field("auction", "Int32"), field("bidder", "Int32"), field("price", "Int32"), field("b_date_time", TS), field("channel", "Utf8")]


def scan(fields):
    return {"execution_plan": "memory_exec", "schema": {"fields": fields, "metadata": {}}, "projection": list(range(len(fields)))}


def find_union(plan):
    """(parent node, key) of the first union_exec on the `input` chain"""
    node = plan
    while node.get("input", {}).get("execution_plan") != "union_exec":
        node = node["input"]
    return node


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--copy-rows", type=int, default=30_000_000)
    ap.add_argument("--baseline-only", action="store_true", help="only the *-separate workloads (what the parent commit executes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "union", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    from flock_amd import GpuContext, NEXMarkSource, Window
    from flock_amd.runtime import ExecutionContext

    gpu = GpuContext(0)
    g = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid",))
    b = g.bids
    auction, bidder, price, when = (x.cpu().numpy() for x in (b.auction, b.bidder, b.price, b.b_date_time))
    del g, b
    n = len(price)
    bid_rb = pa.record_batch([pa.array(auction), pa.array(bidder), pa.array(price), pa.array(when).cast(pa.timestamp("ms"))], names=["auction", "bidder", "price", "b_date_time"])
    na = n // 46
    auction_rb = pa.record_batch([pa.array(when[::46][:na]).cast(pa.timestamp("ms")), pa.array(bidder[::46][:na])], names=["a_date_time", "seller"])
    two = json.load(open(os.path.join(PLANS, "bids_two_ranges.json")))
    act = json.load(open(os.path.join(PLANS, "person_activity.json")))
    # (the fixture's instant is the tests' clock; the generator's events have their own: the second branch keeps the later half of these bids)
    after = int(np.median(when))
    two["inputs"][1]["input"]["input"]["predicate"]["right"]["value"]["Int64"] = after
    want_two = [int((price > 9_000_000).sum()), int((when > after).sum())]
    persons = len(set(np.unique(bidder)))
    want_act = [len(np.unique(auction_rb.column(1).to_numpy())), persons]
    out = {"input": {"bids": n, "auctions": na, "two_ranges_rows": want_two, "activity_groups": want_act, "seconds": a.seconds, "eps": a.eps}, "executes": a.executes,
           "recipe": "plan once, feed once, one untimed execute (row counts checked against numpy), then timed executes; *-separate: one plan per branch, every "
                     "result to the host, appended with pyarrow.concat_tables inside the timed region; kernel times from the library's dispatch-bound events "
                     "over two further executes; bytes = output bytes written + source bytes read once"}

    def summary(times):
        return {"ms_mean": round(statistics.mean(times), 4), "ms_min": round(min(times), 4), "ms_median": round(statistics.median(times), 4), "ms_max": round(max(times), 4),
                "ms_all": [round(t, 4) for t in times]}

    def to_host(plans, feeds, want_rows, retain=False):
        """the plans executed one after the other, results to the host and appended there (one plan: its result alone)"""
        ctxs = [ExecutionContext([p], gpu=gpu) for p in plans]
        try:
            for c, f in zip(ctxs, feeds):
                c.feed_data_sources(f)

            def once():
                if retain:
                    return sum(c.plans[0].execute_retain() for c in ctxs)
                parts = [pa.Table.from_batches(c.execute()[0]) for c in ctxs]
                parts = [t.rename_columns(parts[0].column_names) for t in parts]       # (a union takes input 0's names)
                return (pa.concat_tables(parts) if len(parts) > 1 else parts[0]).num_rows
            rows = once()
            if rows != want_rows:
                raise RuntimeError("%d rows, numpy has %d" % (rows, want_rows))
            for _ in range(2):
                once()
            gpu.synchronize()
            times = []
            for _ in range(a.executes):
                t0 = time.perf_counter()
                once()
                gpu.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            gpu.profile_reset()
            gpu.profile_only(None)
            gpu.profile(True)
            for _ in range(2):
                once()
            gpu.synchronize()
            stats = gpu.profile_read()
            samples = {k: gpu.profile_samples(k) for k in stats if k.startswith("union_")}
            gpu.profile(False)
        finally:
            for c in ctxs:
                c.close()
        e = summary(times)
        e["launches_per_execute"] = sum(v["launches"] for v in stats.values()) / 2
        e["kernels_ms_per_execute"] = {k: round(v["total_ms"] / 2, 4) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])[:12]}
        return e, samples

    def rate(ms, nbytes):
        return {"ms": round(ms, 4), "bytes": int(nbytes), "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1), "frac_of_hbm_peak": round(nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}

    def run(key, fn):
        try:
            e = fn()
        except Exception as ex:   # (a workload that fails is reported, the others still run)
            e = {"error": repr(ex)}
        out[key] = e
        print(key, json.dumps(e), flush=True)

    bid_feed, auction_feed = [[[bid_rb]]], [[[auction_rb]]]
    run("U-two-ranges-separate", lambda: to_host(two["inputs"], [bid_feed, bid_feed], sum(want_two))[0])

    def act_branch(k):
        p = copy.deepcopy(act)
        branch = copy.deepcopy(p_inputs[k])
        names = [f["name"] for f in find_union(act)["input"]["schema"]["fields"]]     # (a union takes input 0's names: alone, the branch carries them itself)
        for pair, f, name in zip(branch["expr"], branch["schema"]["fields"], names):
            pair[1] = f["name"] = name
        find_union(p)["input"] = branch
        return p
    p_inputs = find_union(act)["input"]["inputs"]
    run("U-activity-separate", lambda: to_host([act_branch(0), act_branch(1)], [auction_feed, bid_feed], sum(want_act))[0])
    if not a.baseline_only:
        run("U-two-ranges", lambda: to_host([two], [bid_feed], sum(want_two))[0])
        run("U-activity", lambda: to_host([act], [[[[auction_rb]], [[bid_rb]]]], sum(want_act))[0])

        def w_copy():
            m = min(a.copy_rows, n)
            text = pa.array(np.char.add("ch", np.char.zfill((auction[:m] % 10**9).astype(str), 10)))     # 12 bytes each
            if isinstance(text, pa.ChunkedArray):
                text = text.combine_chunks()
            rb = pa.record_batch([bid_rb.column(i).slice(0, m) for i in range(4)] + [text], names=[f["name"] for f in BID5])
            e, samples = to_host([{"execution_plan": "union_exec", "inputs": [scan(BID5), scan(BID5)]}], [[[[rb]], [[rb]]]], 2 * m, retain=True)
            e["shape"] = {"rows_per_input": m, "inputs": 2, "utf8_bytes_per_value": 12}
            fixed = samples.get("union_fixed_kernel", [])
            per = 4                                                        # launches per execute: auction, bidder, price (4 bytes), b_date_time (8)
            e["kernels"] = {}
            if len(fixed) >= per:
                e["kernels"]["fixed_int32"] = rate(statistics.median(fixed[0::per] + fixed[1::per] + fixed[2::per]), 2 * 4.0 * 2 * m)
                e["kernels"]["fixed_int64"] = rate(statistics.median(fixed[3::per]), 2 * 8.0 * 2 * m)
            if samples.get("union_offsets_kernel"):
                e["kernels"]["offsets"] = rate(statistics.median(samples["union_offsets_kernel"]), 2 * 4.0 * 2 * m)
            if samples.get("union_bytes_kernel"):
                e["kernels"]["bytes"] = rate(statistics.median(samples["union_bytes_kernel"]), 2 * 12.0 * 2 * m)
            return e
        run("U-copy", w_copy)
        for k in ("U-two-ranges", "U-activity"):
            u, p = out.get(k, {}), out.get(k + "-separate", {})
            if "ms_mean" in u and "ms_mean" in p:
                u["vs_separate_plans"] = {"separate_ms_median": p["ms_median"], "ms_median": u["ms_median"], "ratio_of_medians": round(p["ms_median"] / u["ms_median"], 2),
                                          "separate_spread_ms": round(p["ms_max"] - p["ms_min"], 4)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else v.get("ms_median", v.get("error"))) for k, v in out.items() if k != "input"}))
    gpu.close()
    if any(isinstance(v, dict) and "error" in v for v in out.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
