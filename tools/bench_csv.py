"""CSV ingest on the device against the JSON ingest over the SAME rows, in one process, and against pyarrow.csv on the host.

The rows are the ones bench.py's JSON ingest row decodes (`json_side`: the bids of 2e5 generated events, laid end to end 100 times: 1.84e7 rows), written
once as CSV ('auction,bidder,price,b_date_time' under a header) and once as the serde_json lines.  Per format: the whole decode (wall time per call, the
library's own result columns borrowed), every kernel by the library's dispatch-bound events, rows/s, and per kernel the fraction of the 8 TB/s HBM peak
its ALGORITHMIC bytes amount to (the text a pass reads plus what it writes; no counter was read).  Warm-up calls first, medians reported
(measuring-on-mi355x: clocks ramp, the first calls allocate).  Writes one JSON document (default profiles/csv/bench.json) and prints it.

    python tools/bench_csv.py [--steps 20] [--warmup 5] [--copies 100] [--out profiles/csv/bench.json]"""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
BID_CSV = [("auction", "int32"), ("bidder", "int32"), ("price", "int32"), ("b_date_time", "int64")]


def device_text(torch, ctx, head, block, copies):
    n = len(head) + len(block) * copies
    t = torch.zeros(n + 16, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    if head:
        t[: len(head)] = torch.frombuffer(bytearray(head), dtype=torch.uint8).cuda()
    t[len(head): n] = torch.frombuffer(bytearray(block), dtype=torch.uint8).cuda().repeat(copies)
    return t[:n]


def measure(torch, ctx, call, steps, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    walls = []
    for _ in range(steps):                     # plain calls: nothing bracketed
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    ctx.profile_reset()
    ctx.profile_only(None)
    ctx.profile(True)
    for _ in range(steps):                     # the same calls again with every launch bracketed: the kernels' own durations
        call()
    torch.cuda.synchronize()
    stats = ctx.profile_read()
    kernels = {}
    for k, v in stats.items():
        smp = sorted(ctx.profile_samples(k))
        kernels[k] = {"launches_per_call": round(v["launches"] / steps, 2), "median_ms": round(statistics.median(smp), 4) if smp else None,
                      "min_ms": round(smp[0], 4) if smp else None, "max_ms": round(smp[-1], 4) if smp else None,
                      "ms_per_call": round(v["total_ms"] / steps, 4)}
    ctx.profile(False)
    return {"wall_ms": {"median": round(statistics.median(walls), 3), "min": round(min(walls), 3), "max": round(max(walls), 3), "n": steps}, "kernels": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--copies", type=int, default=100)
    ap.add_argument("--block-events", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csv", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from flock_amd import GpuContext, NEXMarkSource, Window
    from flock_amd.nexmark import NEXMARK_JSON_SCHEMAS
    ctx = GpuContext(0)
    g = NEXMarkSource(1, a.block_events, Window.element_wise(), seed=20260926).generate_data(ctx, relations=("bid",))
    cols = {k: getattr(g.bids, k).cpu().numpy() for k, _ in BID_CSV}
    rows_of = list(zip(*(cols[k].tolist() for k, _ in BID_CSV)))
    n_block, rows = len(rows_of), len(rows_of) * a.copies
    head = b"auction,bidder,price,b_date_time\n"
    csv_block = b"".join(b"%d,%d,%d,%d\n" % r for r in rows_of)
    json_block = b"".join(b'{"auction":%d,"bidder":%d,"price":%d,"b_date_time":%d}\n' % r for r in rows_of)
    csv_text = device_text(torch, ctx, head, csv_block, a.copies)
    json_text = device_text(torch, ctx, b"", json_block, a.copies)

    def check(got, n):
        ok = n == rows
        for name, _ in BID_CSV:
            ok = ok and bool((got[name].reshape(a.copies, n_block) == torch.from_numpy(cols[name]).to(got[name].device)).all())
        if not ok:
            raise RuntimeError("the decode differs from the generated columns")

    got, valid, n = ctx.csv_decode(csv_text, BID_CSV, borrow=True)
    check(got, n)
    assert valid == {}
    got, n = ctx.json_lines_decode(json_text, NEXMARK_JSON_SCHEMAS["bid"], borrow=True)
    check(got, n)
    out = {"rows": rows, "steps": a.steps, "warmup": a.warmup, "hbm_peak_bytes_per_s": HBM_PEAK,
           "note": "fractions of the peak are algorithmic bytes (text read by the pass + what it writes) / the kernel's median duration / 8 TB/s"}
    csv_m = measure(torch, ctx, lambda: ctx.csv_decode(csv_text, BID_CSV, borrow=True), a.steps, a.warmup)
    json_m = measure(torch, ctx, lambda: ctx.json_lines_decode(json_text, NEXMARK_JSON_SCHEMAS["bid"], borrow=True), a.steps, a.warmup)
    nb, col_bytes = csv_text.numel(), rows * (4 + 4 + 4 + 8)
    alg = {"csv_index_count_kernel": nb + nb // 4, "csv_index_emit_kernel": nb // 4 + 4 * rows, "csv_parse_kernel": nb + 4 * rows + col_bytes + 4 * rows}
    for k, b in alg.items():
        if k in csv_m["kernels"] and csv_m["kernels"][k]["median_ms"]:
            csv_m["kernels"][k]["algorithmic_bytes"] = int(b)
            csv_m["kernels"][k]["frac_of_hbm_peak"] = round(b / (csv_m["kernels"][k]["median_ms"] * 1e-3) / HBM_PEAK, 4)
    jb = json_text.numel()
    jalg = {"json_newline_count_kernel": jb + jb // 8, "json_newline_emit_kernel": jb // 8 + 4 * rows, "json_parse_kernel": jb + 4 * rows + col_bytes}
    for k, b in jalg.items():
        if k in json_m["kernels"] and json_m["kernels"][k]["median_ms"]:
            json_m["kernels"][k]["algorithmic_bytes"] = int(b)
            json_m["kernels"][k]["frac_of_hbm_peak"] = round(b / (json_m["kernels"][k]["median_ms"] * 1e-3) / HBM_PEAK, 4)
    for name, m, nbytes in (("csv", csv_m, nb), ("json", json_m, jb)):
        m["text_bytes"] = int(nbytes)
        m["bytes_per_row"] = round(nbytes / rows, 2)
        m["rows_per_s"] = round(rows / (m["wall_ms"]["median"] * 1e-3))
        m["kernel_ms_per_call"] = round(sum(v["ms_per_call"] for v in m["kernels"].values()), 4)
        out[name] = m
    out["csv_vs_json_rows_per_s"] = round(out["csv"]["rows_per_s"] / out["json"]["rows_per_s"], 3)
    try:                                        # the host: Arrow C++'s CSV reader (its own thread pool) over ten copies of the block
        import pyarrow as pa
        import pyarrow.csv as pacsv
        sample = head + csv_block * 10
        types = {"auction": pa.int32(), "bidder": pa.int32(), "price": pa.int32(), "b_date_time": pa.int64()}
        best = None
        for _ in range(5):
            t0 = time.perf_counter()
            tb = pacsv.read_csv(io.BytesIO(sample), convert_options=pacsv.ConvertOptions(column_types=types))
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        assert tb.num_rows == n_block * 10 and np.array_equal(tb["auction"].to_numpy()[:n_block], cols["auction"])
        out["pyarrow_csv_host"] = {"rows": tb.num_rows, "best_s": round(best, 4), "rows_per_s": round(tb.num_rows / best), "threads": pa.cpu_count(),
                                   "pyarrow": pa.__version__}
    except ImportError:
        out["pyarrow_csv_host"] = None
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))
    ctx.close()


if __name__ == "__main__":
    main()
