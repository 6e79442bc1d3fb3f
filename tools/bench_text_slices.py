"""Text slice functions (textslice.hpp A-SL1..A-SL8) on the inputs of bench.py's arch_ops: 6e6 auctions (100 s of NEXMark events at 1e6 events/s) with an
item_name of 10-29 bytes, blanks at both ends, and a description of 50-99 bytes of words -- about 450 MB.  Each workload is planned once, fed once, executed
once untimed (its result is checked against pyarrow.compute on the host, which is also timed, for scale) and then --executes times with the result kept in
HBM (flockgpu_plan_execute_retain).  Reported per workload: ms per execute (host clock around execute + synchronise) as min / median / max, and per kernel
its time from the library's dispatch-bound events, its algorithmic bytes from the shapes and its share of the 8 TB/s HBM peak.  Writes
profiles/text_slices/bench.json (or --out).

  row            statement                                                     kernel of interest
  S-split        SELECT split_part(description, ' ', 3)                         text_slice_stream_kernel   (class: the byte equals the delimiter)
  S-right        SELECT right(description, 8)                                   text_slice_stream_kernel   (class: lead bytes; k per row, from utf8_chars_kernel)
  S-btrim        SELECT btrim(item_name)                                        text_slice_stream_kernel   (class: not in the set)
  S-split-2byte  SELECT split_part(description, 'e ', 2)                        text_slice_general_kernel  (one lane per row)
  Y-charlen      SELECT a_id WHERE char_length(description) > 80                utf8_chars_kernel          (the same bytes, no selection step)
  Y-contains     SELECT a_id WHERE description LIKE '%<needle>%'                strmatch_contains_kernel   (the same bytes)

Algorithmic bytes over R rows of a column of B bytes: the streaming slice kernel reads 4 (R + 1) of offsets and B bytes and writes 8 R (S-right: 4 R of
counts more, and utf8_chars_kernel the same bytes once before it); the general kernel the same; utf8_chars_kernel 4 (R + 1) + B + 4 R; the `%needle%`
kernel 4 (R + 1) + B + R / 8 of flag words."""
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


def field(name, dt, nullable=False):
    return {"data_type": dt, "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


AUC = [field("a_id", "Int32"), field("item_name", "Utf8"), field("description", "Utf8")]


def col(name):
    return {"physical_expr": "column", "name": name, "index": [f["name"] for f in AUC].index(name)}


def lit(kind, v):
    return {"physical_expr": "literal", "value": {kind: v}}


def binop(l, op, r):
    return {"physical_expr": "binary_expr", "left": l, "op": op, "right": r}


def fn(name, rt, *args):
    return {"physical_expr": "scalar_function_expr", "name": name, "args": list(args), "return_type": rt}


def scan():
    return {"execution_plan": "memory_exec", "schema": {"fields": AUC, "metadata": {}}, "projection": list(range(len(AUC)))}


def project(e):
    return {"execution_plan": "projection_exec", "expr": [[e, "x"]], "input": scan(), "schema": {"fields": [field("x", "Utf8", True)], "metadata": {}}}


def filt(pred):
    return {"execution_plan": "projection_exec", "expr": [[col("a_id"), "a_id"]], "schema": {"fields": [field("a_id", "Int32")], "metadata": {}},
            "input": {"execution_plan": "filter_exec", "predicate": pred, "input": scan()}}


def random_text(rng, n, lo, hi, blank_every, pad):
    """n values of lo .. hi - 1 bytes: letters, a blank about every `blank_every` bytes, `pad` blanks at each end."""
    import numpy as np
    import pyarrow as pa
    lens = rng.integers(lo, hi, n).astype(np.int32)
    off = np.zeros(n + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    data = rng.integers(97, 123, int(off[-1]), dtype=np.uint8)
    data[rng.random(len(data)) < 1.0 / blank_every] = 32
    for p in range(pad):
        data[off[:-1] + p] = 32
        data[off[1:] - 1 - p] = 32
    return pa.StringArray.from_buffers(n, pa.py_buffer(off.tobytes()), pa.py_buffer(data.tobytes())), int(off[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_slices", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    import pyarrow.compute as pc
    from flock_amd import GpuContext
    from flock_amd.runtime import ExecutionContext

    gpu = GpuContext(0)
    rng = np.random.default_rng(11)
    n = a.seconds * a.eps // 50 * 3
    name, name_bytes = random_text(rng, n, 10, 30, 9, 2)
    desc, desc_bytes = random_text(rng, n, 50, 100, 6, 0)
    rb = pa.record_batch([pa.array(np.arange(n, dtype=np.int32)), name, desc], names=[f["name"] for f in AUC])
    needle = desc[12345].as_py()[20:23]

    def host_split(d, k):   # field k of every value, '' where there are fewer
        one = pc.list_slice(pc.split_pattern(desc, pattern=d), k - 1, k)
        has = pc.equal(pc.list_value_length(one), 1)
        return pc.replace_with_mask(pa.repeat(pa.scalar("", pa.string()), n), has, pc.list_flatten(one).cast(pa.string()))

    offs = 4.0 * (n + 1)
    # name: (plan, kernel of interest, algorithmic bytes of that kernel, host twin or expected row count)
    W = {"S-split": (project(fn("split_part", "Utf8", col("description"), lit("Utf8", " "), lit("Int64", 3))), "text_slice_stream_kernel", offs + desc_bytes + 8.0 * n,
                     lambda: host_split(" ", 3)),
         "S-right": (project(fn("right", "Utf8", col("description"), lit("Int64", 8))), "text_slice_stream_kernel", offs + desc_bytes + 12.0 * n,
                     lambda: pc.utf8_slice_codeunits(desc, -8)),
         "S-btrim": (project(fn("btrim", "Utf8", col("item_name"))), "text_slice_stream_kernel", offs + name_bytes + 8.0 * n, lambda: pc.utf8_trim(name, characters=" ")),
         "S-split-2byte": (project(fn("split_part", "Utf8", col("description"), lit("Utf8", "e "), lit("Int64", 2))), "text_slice_general_kernel", offs + desc_bytes + 8.0 * n,
                           lambda: host_split("e ", 2)),
         "Y-charlen": (filt(binop(fn("char_length", "Int32", col("description")), "Gt", lit("Int32", 80))), "utf8_chars_kernel", offs + desc_bytes + 4.0 * n,
                       lambda: int(pc.sum(pc.greater(pc.utf8_length(desc), 80)).as_py())),
         "Y-contains": (filt(binop(col("description"), "Like", lit("Utf8", "%" + needle + "%"))), "strmatch_contains_kernel", offs + desc_bytes + n / 8.0,
                        lambda: int(pc.sum(pc.match_substring(desc, needle)).as_py()))}
    out = {"input": {"auctions": int(n), "description_bytes": desc_bytes, "item_name_bytes": name_bytes, "seconds": a.seconds, "eps": a.eps}, "executes": a.executes,
           "recipe": "plan once, feed once, one untimed and N timed executes with the result retained in HBM; kernel times from the library's dispatch-bound events"}
    failed = False
    for wname, (plan, kernel, alg, host) in W.items():
        if a.only and wname not in a.only.split(","):
            continue
        e = {}
        ctx = ExecutionContext([plan], gpu=gpu, generic_only=True)
        try:
            t0 = time.perf_counter()
            want = host()
            e["pyarrow_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            ctx.feed_data_sources([[[rb]]])
            got = ctx.execute()[0][0]      # (the untimed execute: arena growth; its result is checked)
            if isinstance(want, int):
                if got.num_rows != want:
                    raise RuntimeError(f"{wname}: {got.num_rows} rows, pyarrow finds {want}")
            else:
                want = want.combine_chunks() if isinstance(want, pa.ChunkedArray) else want
                if not got.column(0).equals(want.cast(pa.string())):
                    raise RuntimeError(f"{wname}: the result differs from pyarrow.compute")
                e["result_bytes"] = int(pc.sum(pc.binary_length(got.column(0))).as_py())
            e["rows_out"] = got.num_rows
            del got, want
            p = ctx.plans[0]
            gpu.synchronize()
            ts = []
            for _ in range(a.executes):
                t0 = time.perf_counter()
                p.execute_retain()
                gpu.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            gpu.profile_reset()
            gpu.profile_only(None)
            gpu.profile(True)
            for _ in range(4):
                p.execute_retain()
            gpu.synchronize()
            stats = gpu.profile_read()
            gpu.profile(False)
            st = stats.get(kernel)
            if not st or not st["launches"]:
                raise RuntimeError(f"{wname}: {kernel} was not launched")
            kms = st["total_ms"] / 4
            e.update({"ms_per_execute": {"min": round(min(ts), 4), "median": round(statistics.median(ts), 4), "max": round(max(ts), 4)},
                      "kernel": kernel, "kernel_ms_per_execute": round(kms, 4), "algorithmic_bytes": int(alg), "GB_per_s": round(alg / (kms * 1e-3) / 1e9, 1),
                      "frac_of_hbm_peak": round(alg / (kms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                      "all_kernels_ms_per_execute": {k: round(v["total_ms"] / 4, 4) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["total_ms"])[:10]}})
        except Exception as ex:   # (a workload that fails is reported, the others still run)
            e["error"] = repr(ex)
            failed = True
        finally:
            ctx.close()
        out[wname] = e
    gpu.close()
    for s in ("S-split", "S-right", "S-btrim"):
        if "frac_of_hbm_peak" in out.get(s, {}) and "frac_of_hbm_peak" in out.get("Y-charlen", {}):
            out[s]["kernel_ms_over_charlen"] = round(out[s]["kernel_ms_per_execute"] / out["Y-charlen"]["kernel_ms_per_execute"], 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
