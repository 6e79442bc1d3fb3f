"""CAST(x AS Int64 / Int32 / Timestamp(ms)) of Utf8 values (textnum.hpp A-TN1..A-TN6) on the inputs of bench.py's arch_ops: 100 s of NEXMark events at 1e6
events/s -- 9.2e7 bids.  The text of `price` and of `b_date_time` is made once (pyarrow.compute.cast on the host, the bytes numtext.hpp writes), uploaded
once as a Utf8 column and kept in HBM.  Each workload is planned once, fed once, executed once untimed (its result is checked against the numbers the text
was made of) and then --executes times ALTERNATING with its yardsticks, all results kept in HBM (flockgpu_plan_execute_retain):
  * utf8_chars_kernel (`char_length(x)`) on the same column: the same stream of offsets and bytes through LDS without the parse;
  * numtext_emit_kernel (`CAST(v AS Utf8)`) on the same rows: the way there.
pyarrow.compute.cast of the text on the host is timed once, for scale.  Reported per workload: ms per execute (host clock around execute + synchronise) as
min / median / max, and per kernel its time from the library's dispatch-bound events, its algorithmic bytes from the shapes and its share of the 8 TB/s HBM
peak.  There is no pass mark.  Writes profiles/parse_text/bench.json (or --out).

  row        statement
  P-price    SELECT CAST(x AS Int64)             x = the text of price
  P-time     SELECT CAST(x AS Timestamp(ms))     x = the text of b_date_time
  P-slice    SELECT CAST(left(x, 4) AS Int32)    x = the text of price

Algorithmic bytes, R rows, B text bytes, V bytes per value written: textnum_parse_kernel reads 4 (R + 1) of offsets and B bytes ONCE (P-slice: 8 R of slice
pairs more) and writes V R of values and R validity bytes; utf8_chars_kernel reads the same 4 (R + 1) + B and writes 4 R; numtext_emit_kernel reads W R of
source values and writes 4 (R + 1) + B."""
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


def col(fields, name):
    return {"physical_expr": "column", "name": name, "index": [f["name"] for f in fields].index(name)}


def lit(kind, v):
    return {"physical_expr": "literal", "value": {kind: v}}


def scan(fields):
    return {"execution_plan": "memory_exec", "schema": {"fields": fields, "metadata": {}}, "projection": list(range(len(fields)))}


def project(fields, e, dt):
    return {"execution_plan": "projection_exec", "expr": [[e, "y"]], "input": scan(fields), "schema": {"fields": [field("y", dt, True)], "metadata": {}}}


def cast(e, dt):
    return {"physical_expr": "cast_expr", "expr": e, "cast_type": dt}


def fn(name, args, rt):
    return {"physical_expr": "scalar_function_expr", "name": name, "args": args, "return_type": rt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parse_text", "bench.json"))
    a = ap.parse_args()
    import pyarrow as pa
    import pyarrow.compute as pc
    from flock_amd import GpuContext, NEXMarkSource, Window
    from flock_amd.runtime import ExecutionContext

    gpu = GpuContext(0)
    g = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid",))
    price = pa.array(g.bids.price.cpu().numpy())
    when = pa.array(g.bids.b_date_time.cpu().numpy()).cast(pa.timestamp("ms"))
    del g
    price_text = pc.cast(price, pa.string())
    when_text = pc.replace_substring_regex(pc.cast(when, pa.string()), r"\.000$", "")   # (pyarrow always prints the millisecond part; numtext.hpp drops a '.000')
    X = [field("x", "Utf8")]
    x = col(X, "x")
    # name: (the parse, its result type, the text column, the host's cast and its Arrow type, the numbers the text was made of, their plan's field, V, W, pair bytes per row)
    W = {"P-price": (cast(x, "Int64"), "Int64", price_text, pa.int64(), price.cast(pa.int64()), field("v", "Int32"), 8, 4, 0),
         "P-time": (cast(x, TS), TS, when_text, pa.timestamp("ms"), when, field("v", TS), 8, 8, 0),
         "P-slice": (cast(fn("left", [x, lit("Int64", 4)], "Utf8"), "Int32"), "Int32", price_text, None, None, field("v", "Int32"), 4, 4, 8)}
    out = {"input": {"bids": len(price), "seconds": a.seconds, "eps": a.eps}, "executes": a.executes,
           "recipe": "plan once, feed once, one untimed and N timed executes alternating with the yardsticks (char_length of the same column; CAST to Utf8 of the same rows), results "
                     "retained in HBM; kernel times from the library's dispatch-bound events"}
    failed = False
    for name, (parse, dt, text, host_ty, source, vfield, V, Wsrc, pair) in W.items():
        if a.only and name not in a.only.split(","):
            continue
        e = {}
        ctx = ExecutionContext([project(X, parse, dt)], gpu=gpu, generic_only=True)
        chars = ExecutionContext([project(X, fn("char_length", [x], "Int32"), "Int32")], gpu=gpu, generic_only=True)
        there = ExecutionContext([project([vfield], cast(col([vfield], "v"), "Utf8"), "Utf8")], gpu=gpu, generic_only=True)
        try:
            text_rb = pa.record_batch([text], names=["x"])
            if host_ty is not None:
                t0 = time.perf_counter()
                want = pc.cast(text, host_ty)
                e["pyarrow_cast_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                if not want.equals(source):
                    raise RuntimeError(f"{name}: pyarrow's cast of the text is not the numbers it was made of")
            else:
                want = pc.cast(pc.utf8_slice_codeunits(text, 0, 4), pa.int32())
            ctx.feed_data_sources([[[text_rb]]])
            got = ctx.execute()[0][0].column(0)      # (the untimed execute: arena growth; its result is checked, value for value)
            if got.null_count or not got.equals(want):
                raise RuntimeError(f"{name}: the result differs from the host's")
            chars.feed_data_sources([[[text_rb]]])
            if not chars.execute()[0][0].column(0).equals(pc.utf8_length(text)):
                raise RuntimeError(f"{name}: char_length differs from the host's")
            src = price if vfield["data_type"] == "Int32" else when
            there.feed_data_sources([[[pa.record_batch([src], names=["v"])]]])
            if not there.execute()[0][0].column(0).equals(price_text if vfield["data_type"] == "Int32" else when_text):
                raise RuntimeError(f"{name}: CAST to Utf8 differs from the text")
            rows, nbytes = len(text), int(pc.sum(pc.binary_length(text)).as_py())
            del got, want
            pairs = ((ctx.plans[0], "ms_per_execute"), (chars.plans[0], "char_length_ms_per_execute"), (there.plans[0], "cast_to_utf8_ms_per_execute"))
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
            alg = {"textnum_parse_kernel": 4.0 * (rows + 1) + nbytes + float(pair) * rows + float(V) * rows + rows, "utf8_chars_kernel": 4.0 * (rows + 1) + nbytes + 4.0 * rows,
                   "numtext_emit_kernel": float(Wsrc) * rows + 4.0 * (rows + 1) + nbytes}
            kernels = {}
            for k, bytes_ in alg.items():
                st = stats.get(k)
                if st and st["launches"]:
                    kms = st["total_ms"] / 4
                    kernels[k] = {"ms_per_execute": round(kms, 4), "algorithmic_bytes": int(bytes_), "GB_per_s": round(bytes_ / (kms * 1e-3) / 1e9, 1),
                                  "frac_of_hbm_peak": round(bytes_ / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
            e.update({"rows": rows, "text_bytes": nbytes, "kernels": kernels,
                      "all_kernels_ms_per_execute": {k: round(v["total_ms"] / 4, 4) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])[:10]}})
        except Exception as ex:   # (a workload that fails is reported, the others still run)
            e["error"] = repr(ex)
            failed = True
        finally:
            there.close()
            chars.close()
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
