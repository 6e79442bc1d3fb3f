"""CAST(x AS Utf8) of integers and timestamps (numtext.hpp A-NT1..A-NT7) on the inputs of bench.py's arch_ops: 100 s of NEXMark events at 1e6 events/s --
9.2e7 bids.  Each workload is planned once, fed once, executed once untimed (its result is checked against pyarrow.compute.cast on the host, which is also
timed, for scale) and then --executes times ALTERNATING with its yardstick, both results kept in HBM (flockgpu_plan_execute_retain): text_select's emit of
a Utf8 column of the same rows and the same bytes -- `CASE WHEN keep >= 0 THEN x END` over the cast's own result (textsel_len_kernel, tile scan,
textsel_emit_kernel, or textsel_emit_long_kernel where a tile's bytes exceed the stage: 1024 timestamps do).  Reported per workload: ms per execute (host
clock around execute + synchronise) as min / median / max for both, and per kernel its time from the library's dispatch-bound events, its algorithmic
bytes from the shapes and its share of the 8 TB/s HBM peak.  Writes profiles/cast_text/bench.json (or --out).

  row        statement
  C-price    SELECT CAST(price AS Utf8)                                                                    (bids)
  C-time     SELECT CAST(b_date_time AS Utf8)                                                              (bids)
  C-q10      SELECT auction, bidder, price, b_date_time, left(CAST(b_date_time AS Utf8), 10), right(left(CAST(b_date_time AS Utf8), 16), 5)
             (tests/golden/plans/q10_date_time_text.json; the whole execute only)

Algorithmic bytes, R rows of W bytes each and B result bytes -- the output written plus the source read ONCE: numtext_len_kernel reads W R (it writes 16
bytes per 1024 rows); numtext_emit_kernel reads W R and writes 4 (R + 1) of offsets and B bytes.  The yardstick: textsel_len_kernel reads the selector and
the column's offsets, 4 R + 8 R; its emit the same again, B source bytes, and writes 4 (R + 1) + B (tiles beyond the stage: textsel_emit_kernel writes the
offsets only, textsel_emit_long_kernel reads 12 R + B and writes B)."""
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


def cast_utf8(e):
    return {"physical_expr": "cast_expr", "expr": e, "cast_type": "Utf8"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cast_text", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    import pyarrow.compute as pc
    from flock_amd import GpuContext, NEXMarkSource, Window
    from flock_amd.runtime import ExecutionContext

    gpu = GpuContext(0)
    g = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid",))
    cols = [g.bids.auction.cpu().numpy(), g.bids.bidder.cpu().numpy(), g.bids.price.cpu().numpy(), g.bids.b_date_time.cpu().numpy()]
    del g
    n_bid = len(cols[0])
    bid_rb = pa.record_batch([pa.array(cols[0]), pa.array(cols[1]), pa.array(cols[2]), pa.array(cols[3]).cast(pa.timestamp("ms"))], names=[f["name"] for f in BID])

    def host_time():   # (pyarrow always prints the millisecond part; chrono drops a '.000')
        return pc.replace_substring_regex(pc.cast(bid_rb.column(3), pa.string()), r"\.000$", "")

    # name: (plan, host twin of the result column or None, bytes per source value, result column)
    W = {"C-price": (project(BID, cast_utf8(col(BID, "price"))), lambda: pc.cast(bid_rb.column(2), pa.string()), 4, 0),
         "C-time": (project(BID, cast_utf8(col(BID, "b_date_time"))), host_time, 8, 0),
         "C-q10": (open(os.path.join(ROOT, "tests", "golden", "plans", "q10_date_time_text.json")).read(), lambda: pc.utf8_slice_codeunits(host_time(), 0, 10), 8, 4)}
    yard_plan = project(YARD, {"physical_expr": "case_expr", "expr": None, "when_then_expr": [[binop(col(YARD, "keep"), "GtEq", lit("Int32", 0)), col(YARD, "x")]], "else_expr": None})
    out = {"input": {"bids": int(n_bid), "seconds": a.seconds, "eps": a.eps}, "executes": a.executes,
           "recipe": "plan once, feed once, one untimed and N timed executes alternating with the yardstick (text_select's emit of the result as a Utf8 column), results retained in HBM; "
                     "kernel times from the library's dispatch-bound events"}
    failed = False
    for name, (plan, host, width, out_col) in W.items():
        if a.only and name not in a.only.split(","):
            continue
        e = {}
        ctx = ExecutionContext([plan], gpu=gpu, generic_only=True)
        yard = ExecutionContext([yard_plan], gpu=gpu, generic_only=True)
        try:
            t0 = time.perf_counter()
            want = host()
            e["pyarrow_cast_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            want = want.combine_chunks() if isinstance(want, pa.ChunkedArray) else want
            ctx.feed_data_sources([[[bid_rb]]])
            got = ctx.execute()[0][0].column(out_col)      # (the untimed execute: arena growth; its result is checked, value for value)
            if not got.equals(want.cast(pa.string())):
                raise RuntimeError(f"{name}: the result differs from pyarrow's cast")
            rows, nbytes = len(got), int(pc.sum(pc.binary_length(got)).as_py())
            whole = name == "C-q10"
            if not whole:
                yard.feed_data_sources([[[pa.record_batch([pa.array(np.zeros(rows, np.int32)), got], names=["keep", "x"])]]])
                if not yard.execute()[0][0].column(0).equals(got):
                    raise RuntimeError(f"{name}: the yardstick does not return its input")
            del got, want
            p_text, p_yard = ctx.plans[0], yard.plans[0]
            pairs = ((p_text, "ms_per_execute"),) if whole else ((p_text, "ms_per_execute"), (p_yard, "yardstick_ms_per_execute"))
            gpu.synchronize()
            times = {key: [] for _, key in pairs}
            for _ in range(a.executes):
                for pl, key in pairs:
                    t0 = time.perf_counter()
                    pl.execute_retain()
                    gpu.synchronize()
                    times[key].append((time.perf_counter() - t0) * 1e3)
            gpu.profile_reset()
            gpu.profile_only(None)
            gpu.profile(True)
            for _ in range(4):
                for pl, _ in pairs:
                    pl.execute_retain()
            gpu.synchronize()
            stats = gpu.profile_read()
            gpu.profile(False)
            for key, ts in times.items():
                e[key] = {"min": round(min(ts), 4), "median": round(statistics.median(ts), 4), "max": round(max(ts), 4)}
            # (the yardstick's tiles of 1024 rows fit text_select's 16 KB stage or they do not -- every value of one workload has about the same length --:
            # the staged kernel then writes the offsets only and the chunk-wise kernel moves the bytes; the kernel that has nothing to move is not rated)
            long_tiles = nbytes / max(rows, 1) * 1024 > 16384
            alg = {"numtext_len_kernel": float(width) * rows, "numtext_emit_kernel": float(width) * rows + 4.0 * (rows + 1) + nbytes,
                   "textsel_len_kernel": 12.0 * rows, "textsel_emit_kernel": 12.0 * rows + 4.0 * (rows + 1) + (0 if long_tiles else 2.0 * nbytes)}
            if long_tiles:
                alg["textsel_emit_long_kernel"] = 12.0 * rows + 2.0 * nbytes
            kernels = {}
            for k, bytes_ in alg.items():
                st = stats.get(k)
                if st and st["launches"] and not whole:
                    kms = st["total_ms"] / 4
                    kernels[k] = {"ms_per_execute": round(kms, 4), "algorithmic_bytes": int(bytes_), "GB_per_s": round(bytes_ / (kms * 1e-3) / 1e9, 1),
                                  "frac_of_hbm_peak": round(bytes_ / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
            e.update({"rows": rows, "result_bytes": nbytes, "kernels": kernels,
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
