"""Utf8-valued expressions (textsel.hpp A-T1..A-T5) on the inputs of bench.py's arch_ops: 100 s of NEXMark events at 1e6 events/s -- 9.2e7 bids, and 6e6
auctions with an item_name of 10-29 bytes and a description of 50-99 bytes.  Each workload is planned once, fed once, executed once untimed (its result is
checked against pyarrow's case_when on the host, which is also timed, for scale) and then --executes times ALTERNATING with its yardstick, both results
kept in HBM (flockgpu_plan_execute_retain): the project's own take of a Utf8 column that produces the same rows and the same output bytes -- the result
column itself under a filter that keeps every row (utf8_len_kernel, tile scan, utf8_emit_kernel / utf8_emit_long_kernel).  Reported per workload: ms per
execute (host clock around execute + synchronise) as min / median / max for both, and per kernel its time from the library's dispatch-bound events, its
algorithmic bytes from the shapes and its share of the 8 TB/s HBM peak.  Writes profiles/text_expr/bench.json (or --out).

  row           statement
  T-q14         SELECT CASE WHEN date_part('hour', t) BETWEEN 8 AND 18 THEN 'dayTime' WHEN ... <= 6 OR ... >= 20 THEN 'nightTime' ELSE 'otherTime' END   (bids)
  T-q14-hours   the same over the same bids with their timestamps moved to all 24 hours (the 100 s of the arch_ops input lie in ONE hour: T-q14 writes
                one label, 'otherTime', for every row)
  T-two-cols    SELECT CASE WHEN reserve > 0 THEN item_name ELSE description END                                                                        (auctions)
  T-literal     SELECT 'bid'                                                                                                                            (bids; reported only)

Algorithmic bytes, R rows and B result bytes: textsel_len_kernel reads the selector, 4 R (and the two offsets of the chosen column, 8 R, when sources are
columns); textsel_emit_kernel reads the selector again and writes 4 (R + 1) of offsets and B bytes (columns: 8 R of offsets and B source bytes more;
with tiles beyond the stage it writes the offsets only and textsel_emit_long_kernel reads selector, offsets and source bytes and writes B).  The
take: utf8_len_kernel 4 R of row numbers + 8 R of offsets, the emit the same again + 4 (R + 1) + 2 B."""
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


BID = [field("price", "Int32"), field("b_date_time", TS)]
AUC = [field("reserve", "Int32"), field("item_name", "Utf8"), field("description", "Utf8")]
YARD = [field("keep", "Int32"), field("x", "Utf8")]


def col(fields, name):
    return {"physical_expr": "column", "name": name, "index": [f["name"] for f in fields].index(name)}


def lit(kind, v):
    return {"physical_expr": "literal", "value": {kind: v}}


def binop(l, op, r):
    return {"physical_expr": "binary_expr", "left": l, "op": op, "right": r}


def scan(fields):
    return {"execution_plan": "memory_exec", "schema": {"fields": fields, "metadata": {}}, "projection": list(range(len(fields)))}


def project(fields, e):
    return {"execution_plan": "projection_exec", "expr": [[e, "x"]], "input": scan(fields), "schema": {"fields": [field("x", "Utf8", True)], "metadata": {}}}


def case(whens, els):
    return {"physical_expr": "case_expr", "expr": None, "when_then_expr": [[w, t] for w, t in whens], "else_expr": els}


def random_text(rng, n, lo, hi):
    import numpy as np
    import pyarrow as pa
    lens = rng.integers(lo, hi, n).astype(np.int32)
    off = np.zeros(n + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    data = rng.integers(97, 123, int(off[-1]), dtype=np.uint8)
    return pa.StringArray.from_buffers(n, pa.py_buffer(off.tobytes()), pa.py_buffer(data.tobytes()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_expr", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    import pyarrow.compute as pc
    from flock_amd import GpuContext, NEXMarkSource, Window
    from flock_amd.runtime import ExecutionContext

    gpu = GpuContext(0)
    g = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid",))
    price, when = g.bids.price.cpu().numpy(), g.bids.b_date_time.cpu().numpy()
    del g
    bid_rb = pa.record_batch([pa.array(price), pa.array(when).cast(pa.timestamp("ms"))], names=[f["name"] for f in BID])
    n_bid = len(price)
    spread = when + (np.arange(n_bid, dtype=np.int64) * 7 % 24) * 3_600_000
    hours_rb = pa.record_batch([pa.array(price), pa.array(spread).cast(pa.timestamp("ms"))], names=[f["name"] for f in BID])
    rng = np.random.default_rng(11)
    n_auc = a.seconds * a.eps // 50 * 3
    reserve = rng.integers(-5, 6, n_auc).astype(np.int32)
    auc_rb = pa.record_batch([pa.array(reserve), random_text(rng, n_auc, 10, 30), random_text(rng, n_auc, 50, 100)], names=[f["name"] for f in AUC])

    hour = {"physical_expr": "scalar_function_expr", "name": "date_part", "args": [lit("Utf8", "hour"), col(BID, "b_date_time")], "return_type": "Int32"}
    q14 = case([(binop(binop(hour, "GtEq", lit("Int32", 8)), "And", binop(hour, "LtEq", lit("Int32", 18))), lit("Utf8", "dayTime")),
                (binop(binop(hour, "LtEq", lit("Int32", 6)), "Or", binop(hour, "GtEq", lit("Int32", 20))), lit("Utf8", "nightTime"))], lit("Utf8", "otherTime"))
    two = case([(binop(col(AUC, "reserve"), "Gt", lit("Int32", 0)), col(AUC, "item_name"))], col(AUC, "description"))

    def host_q14(rb=None):
        h = pc.hour((bid_rb if rb is None else rb).column(1))
        conds = pa.StructArray.from_arrays([pc.and_(pc.greater_equal(h, 8), pc.less_equal(h, 18)), pc.or_(pc.less_equal(h, 6), pc.greater_equal(h, 20))], names=["a", "b"])
        return pc.case_when(conds, pa.scalar("dayTime"), pa.scalar("nightTime"), pa.scalar("otherTime"))

    def host_two():
        return pc.case_when(pa.StructArray.from_arrays([pc.greater(auc_rb.column(0), 0)], names=["a"]), auc_rb.column(1), auc_rb.column(2))

    # name: (plan, feed, host twin, column sources?)
    W = {"T-q14": (project(BID, q14), bid_rb, host_q14, False),
         "T-q14-hours": (project(BID, q14), hours_rb, lambda: host_q14(hours_rb), False),
         "T-two-cols": (project(AUC, two), auc_rb, host_two, True),
         "T-literal": (project(BID, lit("Utf8", "bid")), bid_rb, lambda: pa.repeat(pa.scalar("bid"), n_bid), False)}
    yard_plan = {"execution_plan": "projection_exec", "expr": [[col(YARD, "x"), "x"]], "schema": {"fields": [field("x", "Utf8", True)], "metadata": {}},
                 "input": {"execution_plan": "filter_exec", "predicate": binop(col(YARD, "keep"), "GtEq", lit("Int32", 0)), "input": scan(YARD)}}
    out = {"input": {"bids": int(n_bid), "auctions": int(n_auc), "seconds": a.seconds, "eps": a.eps}, "executes": a.executes,
           "recipe": "plan once, feed once, one untimed and N timed executes alternating with the yardstick take, results retained in HBM; kernel times from the library's dispatch-bound events"}
    failed = False
    for name, (plan, rb, host, cols) in W.items():
        if a.only and name not in a.only.split(","):
            continue
        e = {}
        ctx = ExecutionContext([plan], gpu=gpu, generic_only=True)
        yard = ExecutionContext([yard_plan], gpu=gpu, generic_only=True)
        try:
            t0 = time.perf_counter()
            want = host()
            e["pyarrow_case_when_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            want = want.combine_chunks() if isinstance(want, pa.ChunkedArray) else want
            ctx.feed_data_sources([[[rb]]])
            got = ctx.execute()[0][0].column(0)      # (the untimed execute: arena growth; its result is checked, value for value)
            if not got.equals(want.cast(pa.string())):
                raise RuntimeError(f"{name}: the result differs from pyarrow's case_when")
            rows, nbytes = len(got), int(pc.sum(pc.binary_length(got)).as_py())
            distinct = int(pc.count_distinct(got.slice(0, 1_000_000)).as_py())      # (of the first 1e6 rows)
            yard.feed_data_sources([[[pa.record_batch([pa.array(np.zeros(rows, np.int32)), got], names=["keep", "x"])]]])
            if not yard.execute()[0][0].column(0).equals(got):
                raise RuntimeError(f"{name}: the yardstick take does not return its input")
            del got, want
            p_text, p_yard = ctx.plans[0], yard.plans[0]
            gpu.synchronize()
            t_text, t_yard = [], []
            for _ in range(a.executes):
                for pl, ts in ((p_text, t_text), (p_yard, t_yard)):
                    t0 = time.perf_counter()
                    pl.execute_retain()
                    gpu.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
            gpu.profile_reset()
            gpu.profile_only(None)
            gpu.profile(True)
            for _ in range(4):
                p_text.execute_retain()
                p_yard.execute_retain()
            gpu.synchronize()
            stats = gpu.profile_read()
            gpu.profile(False)
            ms = lambda ts: {"min": round(min(ts), 4), "median": round(statistics.median(ts), 4), "max": round(max(ts), 4)}
            long_tiles = "textsel_emit_long_kernel" in stats and stats["textsel_emit_long_kernel"]["launches"]
            alg = {"textsel_len_kernel": 4.0 * rows + (8.0 * rows if cols else 0),
                   "textsel_emit_kernel": 8.0 * rows + 4 + (8.0 * rows if cols else 0) + (0 if long_tiles else nbytes + (nbytes if cols else 0)),
                   "textsel_emit_long_kernel": 12.0 * rows + 2.0 * nbytes,
                   "textsel_fill_kernel": 4.0 * rows + 4 + nbytes, "utf8_len_kernel": 12.0 * rows, "utf8_emit_kernel": 16.0 * rows + 4 + 2.0 * nbytes,
                   "utf8_emit_long_kernel": 16.0 * rows + 4 + 2.0 * nbytes}
            kernels = {}
            for k, bytes_ in alg.items():
                st = stats.get(k)
                if st and st["launches"]:
                    kms = st["total_ms"] / 4
                    kernels[k] = {"ms_per_execute": round(kms, 4), "algorithmic_bytes": int(bytes_), "GB_per_s": round(bytes_ / (kms * 1e-3) / 1e9, 1),
                                  "frac_of_hbm_peak": round(bytes_ / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
            e.update({"rows": rows, "result_bytes": nbytes, "distinct_values": distinct, "ms_per_execute": ms(t_text), "yardstick_take_ms_per_execute": ms(t_yard), "kernels": kernels,
                      "all_kernels_ms_per_execute": {k: round(v["total_ms"] / 4, 4) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])[:10]}})
        except Exception as ex:   # (a workload that fails is reported, the others still run)
            e["error"] = repr(ex)
            failed = True
        finally:
            yard.close()
            ctx.close()
        out[name] = e
    gpu.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
