"""Text sinks on the device: columns -> JSON lines and CSV (flockgpu_json_lines_encode / flockgpu_csv_encode, textenc.hip), in one process.

Inputs:
  bids       the rows bench.py's JSON ingest row decodes (the bids of 2e5 generated events, laid end to end 100 times: 1.84e7 rows), as JSON lines and as CSV;
  auctions   6e6 rows (a_id, description) with a description of 50-99 bytes, ~450 MB, as the arch_ops inputs of the other text benchmarks have it: once
             verbatim, once with a '"' in every tenth description (the class pass then finds class bytes and the emit pass escapes / quotes).
Per input and format: the whole encode (wall time per call, the library's own buffer borrowed), every kernel by the library's dispatch-bound events, and per
pass the fraction of the 8 TB/s HBM peak its ALGORITHMIC bytes amount to (the columns a pass reads plus what it writes; no counter was read).  Every text
is decoded again on the device and compared with the columns before anything is timed.  Warm-up calls first, medians reported (measuring-on-mi355x: clocks
ramp, the first calls allocate).  The host baselines run on a tenth of the bid rows: oracle.nexmark_json_lines (a json.dumps per row) and
pyarrow.csv.write_csv.  Writes one JSON document (default profiles/text_encode/bench.json) and prints it.

    python tools/bench_text_encode.py [--steps 20] [--warmup 5] [--copies 100] [--out profiles/text_encode/bench.json]"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_csv import HBM_PEAK, measure  # noqa: E402

BID = [("auction", "int32"), ("bidder", "int32"), ("price", "int32"), ("b_date_time", "int64")]
YARDSTICKS = {"numtext_emit_kernel": "0.40-0.70 of the peak", "union_bytes_kernel": "0.68", "utf8_chars_kernel": "0.33-0.61",
              "flockgpu_json_lines_decode_ms_same_bid_rows": 0.80, "flockgpu_csv_decode_ms_same_bid_rows": 1.32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--copies", type=int, default=100)
    ap.add_argument("--block-events", type=int, default=200_000)
    ap.add_argument("--auctions", type=int, default=6_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_encode", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from flock_amd import DeviceUtf8, GpuContext, NEXMarkSource, Window
    ctx = GpuContext(0)
    dev = f"cuda:{ctx.device}"
    g = NEXMarkSource(1, a.block_events, Window.element_wise(), seed=20260926).generate_data(ctx, relations=("bid",))
    block = {k: getattr(g.bids, k) for k, _ in BID}
    bids = [(k, t, block[k].repeat(a.copies)) for k, t in BID]
    rows = bids[0][2].numel()

    torch.manual_seed(11)
    n_auc = a.auctions
    lens = torch.randint(50, 100, (n_auc,), device=dev, dtype=torch.int32)
    off = torch.zeros(n_auc + 1, dtype=torch.int32, device=dev)
    off[1:] = torch.cumsum(lens, 0)
    n_desc = int(off[-1])
    data = torch.randint(97, 123, (n_desc + 16,), device=dev, dtype=torch.uint8)
    a_id = torch.arange(n_auc, dtype=torch.int32, device=dev)
    quoted = data.clone()
    quoted[(off[:-1][::10] + 20).long()] = 0x22
    inputs = {"bids": (bids, rows), "auctions_verbatim": ([("a_id", "int32", a_id), ("description", "utf8", DeviceUtf8(off, data))], n_auc),
              "auctions_every_tenth_quoted": ([("a_id", "int32", a_id), ("description", "utf8", DeviceUtf8(off, quoted))], n_auc)}

    def same(got, cols, n, n_rows):
        ok = n == n_rows
        for name, t, col in cols:
            if t == "utf8":
                ok = ok and bool((got[name].offsets == col.offsets).all()) and bool((got[name].data[: int(col.offsets[-1])] == col.data[: int(col.offsets[-1])]).all())
            else:
                ok = ok and bool((got[name] == col).all())
        if not ok:
            raise RuntimeError("the text does not decode to the columns it was made from")

    out = {"steps": a.steps, "warmup": a.warmup, "hbm_peak_bytes_per_s": HBM_PEAK, "yardsticks_from_the_readme": YARDSTICKS,
           "note": "fractions of the peak are algorithmic bytes (the columns a pass reads + what it writes) / the kernel's median duration / 8 TB/s"}
    for label, (cols, n_rows) in inputs.items():
        fields = [(name, t) for name, t, _ in cols]
        num = sum(n_rows * (4 if t == "int32" else 8) for _, t, _ in cols if t != "utf8")
        text_in = sum(int(c.offsets[-1]) for _, t, c in cols if t == "utf8")
        n_utf8 = sum(t == "utf8" for _, t, _ in cols)
        entry = {"rows": n_rows, "column_bytes": int(num + text_in + 4 * n_utf8 * n_rows)}
        for fmt, call in (("json", lambda: ctx.json_lines_encode(cols, borrow=True)), ("csv", lambda: ctx.csv_encode(cols, borrow=True))):
            text = call()
            nb = text.numel()
            if fmt == "json":
                got, n = ctx.json_lines_decode(text, fields, borrow=True)
            else:
                got, valid, n = ctx.csv_decode(text, fields, borrow=True)
                assert valid == {}
            same(got, cols, n, n_rows)
            del got
            m = measure(torch, ctx, call, a.steps, a.warmup)
            class_seen = "textenc_class_kernel" in m["kernels"]
            extras = 4 * n_utf8 * n_rows if label.endswith("quoted") else 0          # (a column without class bytes: the extras are not read again)
            alg = {"textenc_class_kernel": text_in + 2 * 4 * n_utf8 * n_rows,
                   "textenc_len_kernel": num + 2 * 4 * n_utf8 * n_rows + extras + 4 * n_rows,
                   "textenc_emit_kernel": num + text_in + 2 * 4 * n_utf8 * n_rows + extras + 4 * n_rows + nb}
            for k, b in alg.items():
                if k in m["kernels"] and m["kernels"][k]["median_ms"]:
                    per_call = m["kernels"][k]["ms_per_call"] if k == "textenc_class_kernel" else m["kernels"][k]["median_ms"]   # (one scope over a launch per Utf8 column)
                    m["kernels"][k]["algorithmic_bytes"] = int(b)
                    m["kernels"][k]["frac_of_hbm_peak"] = round(b / (per_call * 1e-3) / HBM_PEAK, 4)
            m["text_bytes"] = int(nb)
            m["bytes_per_row"] = round(nb / n_rows, 2)
            m["rows_per_s"] = round(n_rows / (m["wall_ms"]["median"] * 1e-3))
            m["text_bytes_per_s"] = round(nb / (m["wall_ms"]["median"] * 1e-3))
            m["kernel_ms_per_call"] = round(sum(v["ms_per_call"] for v in m["kernels"].values()), 4)
            m["class_pass_ran"] = class_seen
            entry[fmt] = m
            del text
        out[label] = entry

    # the host, on a tenth of the bid rows
    host_cols = {k: block[k].cpu().numpy() for k, _ in BID}
    tenth = {k: np.tile(v, max(a.copies // 10, 1)) for k, v in host_cols.items()}
    n_host = len(tenth["auction"])
    try:
        import oracle
        t0 = time.perf_counter()
        text = oracle.nexmark_json_lines("bid", tenth)
        dt = time.perf_counter() - t0
        out["oracle_json_lines_host"] = {"rows": n_host, "seconds": round(dt, 3), "rows_per_s": round(n_host / dt), "text_bytes": len(text)}
    except ImportError:
        out["oracle_json_lines_host"] = None
    try:
        import pyarrow as pa
        import pyarrow.csv as pacsv
        tb = pa.table({k: pa.array(v) for k, v in tenth.items()})
        best = None
        for _ in range(5):
            sink = io.BytesIO()
            t0 = time.perf_counter()
            pacsv.write_csv(tb, sink)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out["pyarrow_write_csv_host"] = {"rows": n_host, "best_s": round(best, 4), "rows_per_s": round(n_host / best), "text_bytes": sink.tell(),
                                         "pyarrow": pa.__version__}
    except ImportError:
        out["pyarrow_write_csv_host"] = None
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))
    ctx.close()


if __name__ == "__main__":
    main()
