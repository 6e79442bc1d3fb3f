"""Utf8 LIKE and ordered Utf8 comparisons (strmatch.hpp) on the inputs of bench.py's arch_ops: 100 s of NEXMark events at 1e6 events/s -- 6e6 auctions
with item_name (8-19 bytes) and description (50-99 bytes, ~450 MB), 2e6 persons with name and state.  Each workload is planned once, fed once and
executed 10 times with its result kept in HBM (flockgpu_plan_execute_retain); reported per workload: ms per execute, kernel launches per execute, and
per new kernel its time, algorithmic bytes and fraction of the 8 TB/s HBM peak.  Writes profiles/like/bench.json (or --out).

Yardsticks, measured by this tool in the same process: pred_flag_kernel's fraction of the peak on arch_filter (the stream); pyarrow.compute on the same
Arrow column on this host, one call, best of 5 (the CPU); L-eq, the existing Utf8 `=` leaf (class (a)).  The row count of every timed workload is checked
against pyarrow's count for the same predicate.

Algorithmic bytes of a string-match kernel over R rows: offsets 4 (R + 1); plus the column's bytes (`%needle%` and the general matcher) or min(value, pattern)
bytes per row (anchored patterns, comparisons); plus 4 bytes per 32 rows of flag words out.

Workloads (the needles are picked from the generated data; selectivity between 0.1 % and 10 %, recorded):
  L-prefix          item_name LIKE '<p>%'
  L-suffix          description LIKE '%<s>'
  L-contains        description LIKE '%<needle>%'        (the headline)
  L-contains-short  state LIKE '%<c>%'
  L-general         description LIKE '%<a>%<b>_<c>%'
  L-range           name >= '<x>' AND name < '<y>'
  L-eq              item_name = '<literal>'              (the existing leaf)
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


def field(name, dt):
    return {"data_type": dt, "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": False}


AUC = [field("a_id", "Int32"), field("item_name", "Utf8"), field("description", "Utf8")]
PER = [field("p_id", "Int32"), field("name", "Utf8"), field("state", "Utf8")]


def col(fields, name):
    return {"physical_expr": "column", "name": name, "index": [f["name"] for f in fields].index(name)}


def lit(s):
    return {"physical_expr": "literal", "value": {"Utf8": s}}


def binop(op, l, r):
    return {"physical_expr": "binary_expr", "op": op, "left": l, "right": r}


def filter_plan(fields, pred):
    scan = {"execution_plan": "memory_exec", "schema": {"fields": fields, "metadata": {}}, "projection": list(range(len(fields)))}
    return {"execution_plan": "filter_exec", "predicate": pred, "input": scan}


NEW_KERNELS = ("strmatch_contains_kernel", "strmatch_rows_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-cpu", action="store_true", help="skip the pyarrow timings (the row counts are still checked)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "like", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    import pyarrow.compute as pc
    from flock_amd import GpuContext
    from flock_amd.runtime import ExecutionContext

    rng = np.random.default_rng(11)
    n_events = a.seconds * a.eps
    n_auc, n_per = n_events // 50 * 3, n_events // 50      # the generator's 46 : 3 : 1 split of bids, auctions and persons

    def words(n, lo, hi):   # strings at the widths of the reference's generator, as bench.py's arch_ops synthesises them
        lens = rng.integers(lo, hi + 1, n).astype(np.int32)
        off = np.zeros(n + 1, np.int32)
        np.cumsum(lens, out=off[1:])
        data = rng.integers(97, 123, int(off[-1]), dtype=np.uint8)
        return pa.StringArray.from_buffers(n, pa.py_buffer(off.tobytes()), pa.py_buffer(data.tobytes()))
    auc_rb = pa.record_batch([pa.array(np.arange(n_auc, dtype=np.int32)), words(n_auc, 8, 19), words(n_auc, 50, 99)], names=[f["name"] for f in AUC])
    per_rb = pa.record_batch([pa.array(np.arange(n_per, dtype=np.int32)), words(n_per, 8, 19), words(n_per, 2, 2)], names=[f["name"] for f in PER])

    def pick(column, make, tries=200):
        """a predicate over `column` with a selectivity between 0.1 % and 10 %: make(sample value) -> (pyarrow mask function, description)"""
        n = len(column)
        for t in range(tries):
            v = column[int(rng.integers(0, n))].as_py()
            cand = make(v)
            sel = pc.sum(cand["mask"](column)).as_py() / n
            if 0.001 <= sel <= 0.10:
                cand["selectivity"] = round(sel, 5)
                return cand
        raise RuntimeError("no needle with a selectivity between 0.1 % and 10 %")

    item, desc, name, state = auc_rb.column("item_name"), auc_rb.column("description"), per_rb.column("name"), per_rb.column("state")
    like_of = lambda pattern: (lambda c: pc.match_like(c, pattern))
    W = {}
    c = pick(item, lambda v: {"pattern": v[:2] + "%", "mask": like_of(v[:2] + "%")})
    W["L-prefix"] = dict(c, fields=AUC, rb=auc_rb, column="item_name", pred=binop("Like", col(AUC, "item_name"), lit(c["pattern"])), klass="a")
    c = pick(desc, lambda v: {"pattern": "%" + v[-2:], "mask": like_of("%" + v[-2:])})
    W["L-suffix"] = dict(c, fields=AUC, rb=auc_rb, column="description", pred=binop("Like", col(AUC, "description"), lit(c["pattern"])), klass="a")
    c = pick(desc, lambda v: {"pattern": "%" + v[20:23] + "%", "mask": like_of("%" + v[20:23] + "%")})
    W["L-contains"] = dict(c, fields=AUC, rb=auc_rb, column="description", pred=binop("Like", col(AUC, "description"), lit(c["pattern"])), klass="b")
    c = pick(state, lambda v: {"pattern": "%" + v[:1] + "%", "mask": like_of("%" + v[:1] + "%")})
    W["L-contains-short"] = dict(c, fields=PER, rb=per_rb, column="state", pred=binop("Like", col(PER, "state"), lit(c["pattern"])), klass="b")
    c = pick(desc, lambda v: {"pattern": "%" + v[5:7] + "%" + v[30] + "_" + v[32] + "%", "mask": like_of("%" + v[5:7] + "%" + v[30] + "_" + v[32] + "%")})
    W["L-general"] = dict(c, fields=AUC, rb=auc_rb, column="description", pred=binop("Like", col(AUC, "description"), lit(c["pattern"])), klass="c")

    def rng_of(v):
        x, y = v[:2], v[:1] + chr(ord(v[1]) + 2) if v[1] < "y" else v[:1] + "{"
        return {"pattern": [x, y], "mask": lambda c: pc.and_(pc.greater_equal(c, x), pc.less(c, y))}
    c = pick(name, rng_of)
    W["L-range"] = dict(c, fields=PER, rb=per_rb, column="name", klass="a",
                        pred=binop("And", binop("GtEq", col(PER, "name"), lit(c["pattern"][0])), binop("Lt", col(PER, "name"), lit(c["pattern"][1]))))
    v = item[int(rng.integers(0, n_auc))].as_py()
    W["L-eq"] = dict(pattern=v, mask=lambda c: pc.equal(c, v), selectivity=None, fields=AUC, rb=auc_rb, column="item_name", klass="eq",
                     pred=binop("Eq", col(AUC, "item_name"), lit(v)))

    gpu = GpuContext(0)
    out = {"input": {"auctions": n_auc, "persons": n_per, "seconds": a.seconds, "eps": a.eps,
                     "bytes": {"item_name": item.buffers()[2].size, "description": desc.buffers()[2].size, "name": name.buffers()[2].size, "state": state.buffers()[2].size}},
           "executes": a.executes,
           "recipe": "plan once, feed once, executes with the result retained in HBM; kernel times from the library's dispatch-bound events (the kernel-trace run beside this file has rocprofv3's)"}

    def timed(plan, feed, n_exec):
        ctx = ExecutionContext([plan], gpu=gpu)
        try:
            ctx.feed_data_sources(feed)
            pl = ctx.plans[0]
            rows = pl.execute_retain()      # (first execute: arena growth)
            gpu.synchronize()
            times = []
            for _ in range(n_exec):
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
        finally:
            ctx.close()
        return int(rows), times, stats

    # ---- the stream's yardstick: arch_filter on the generic operators, the bids of the same events
    if not a.only:
        from flock_amd import NEXMarkSource, Window
        g = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid",))
        b = g.bids
        bid_rb = pa.record_batch([pa.array(b.auction.cpu().numpy()), pa.array(b.bidder.cpu().numpy()), pa.array(b.price.cpu().numpy()),
                                  pa.array(b.b_date_time.cpu().numpy()).cast(pa.timestamp("ms"))], names=["auction", "bidder", "price", "b_date_time"])
        del g, b
        plan = json.load(open(os.path.join(ROOT, "tests", "golden", "plans", "arch_filter.json")))
        ctx = ExecutionContext([plan], gpu=gpu, generic_only=True)
        try:
            ctx.feed_data_sources([[[bid_rb]]])
            pl = ctx.plans[0]
            pl.execute_retain()
            gpu.synchronize()
            gpu.profile_reset()
            gpu.profile_only(None)
            gpu.profile(True)
            for _ in range(4):
                pl.execute_retain()
            gpu.synchronize()
            st = gpu.profile_read()["pred_flag_kernel"]
            gpu.profile(False)
        finally:
            ctx.close()
        ms = st["total_ms"] / 4
        alg = 4.0 * bid_rb.num_rows
        out["yardstick_stream"] = {"kernel": "pred_flag_kernel on arch_filter (generic operators)", "bids": bid_rb.num_rows, "ms_per_execute": round(ms, 4),
                                   "algorithmic_bytes": int(alg), "frac_of_hbm_peak": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        print("yardstick", json.dumps(out["yardstick_stream"]), flush=True)
        del bid_rb

    for wname, w in W.items():
        if a.only and wname not in a.only.split(","):
            continue
        e = {"pattern": w["pattern"], "selectivity": w["selectivity"], "class": w["klass"], "column": w["column"]}
        try:
            column = w["rb"].column(w["column"])
            R = len(column)
            want = pc.sum(w["mask"](column)).as_py()
            if not a.no_cpu:
                best = 1e9
                for _ in range(5):
                    t0 = time.perf_counter()
                    w["mask"](column)
                    best = min(best, time.perf_counter() - t0)
                e["cpu_pyarrow_ms"] = round(best * 1e3, 3)
            rows, times, stats = timed(filter_plan(w["fields"], w["pred"]), [[[w["rb"]]]], a.executes)
            if rows != want:
                raise RuntimeError(f"{wname}: {rows} rows, pyarrow counts {want}")
            e.update({"ms_per_execute": round(sum(times) / len(times) * 1e3, 4), "ms_min": round(min(times) * 1e3, 4), "result_rows": rows, "input_rows": R,
                      "launches_per_execute": sum(v["launches"] for v in stats.values()) / 2,
                      "kernels_ms_per_execute": {k: round(v["total_ms"] / 2, 4) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])[:8]}})
            col_bytes = column.buffers()[2].size
            lens = pc.binary_length(column)
            pat_len = max(len(p) for p in w["pattern"]) if isinstance(w["pattern"], list) else len(w["pattern"].replace("%", ""))
            touched = pc.sum(pc.min_element_wise(lens, pat_len)).as_py()
            alg = 4.0 * (R + 1) + (col_bytes if w["klass"] in ("b", "c") else touched) + 4.0 * R / 32
            new = {}
            for k in NEW_KERNELS + (("pred_flag_kernel",) if w["klass"] == "eq" else ()):
                st = stats.get(k)
                if not st or not st["launches"]:
                    continue
                ms = st["total_ms"] / 2
                launches = st["launches"] / 2
                new[k] = {"ms_per_execute": round(ms, 4), "launches_per_execute": launches, "algorithmic_bytes": int(alg * launches), "GB_per_s": round(alg * launches / (ms * 1e-3) / 1e9, 1),
                          "frac_of_hbm_peak": round(alg * launches / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
            e["new_kernels"] = new
        except Exception as ex:   # (a workload that fails is reported, the others still run)
            e["error"] = repr(ex)
        out[wname] = e
        print(wname, json.dumps(e), flush=True)
    if "yardstick_stream" in out and "new_kernels" in out.get("L-contains", {}) and "strmatch_contains_kernel" in out["L-contains"]["new_kernels"]:
        out["L-contains_over_stream_yardstick"] = round(out["L-contains"]["new_kernels"]["strmatch_contains_kernel"]["frac_of_hbm_peak"] / out["yardstick_stream"]["frac_of_hbm_peak"], 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else v.get("ms_per_execute", v.get("error"))) for k, v in out.items() if k != "input"}))
    gpu.close()
    if any(isinstance(v, dict) and "error" in v for v in out.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
