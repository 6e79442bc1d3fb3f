"""The JSON-lines decoder with NULLs (flockgpu_json_lines_decode_nullable) next to the first decoder over the SAME rows, in one process.

The rows are the ones bench.py's JSON ingest row decodes (the bids of 2e5 generated events, laid end to end 100 times: 1.84e7 rows).  Texts: the serde_json
lines as they are (both decoders); `null` in 10 % of one column and of every column; a member absent in 10 % of the lines (the second kernel); the device
encoder's own output read back.  Every text is decoded and compared with its columns, validity and null counts before anything is timed.  Per text: the whole
decode (wall time per call, result columns borrowed), every kernel by the library's dispatch-bound events, rows/s, and for the parse kernels the fraction of
the 8 TB/s HBM peak their ALGORITHMIC bytes amount to (the text the pass reads plus what it writes; no counter was read).  Warm-up calls first, medians
reported.  --parent-lib: a libflockgpu.so built from the parent commit; its flockgpu_json_lines_decode and this tree's then run alternating on the same
text (parent, this tree, parent again per round); both medians and the spread of the parent against itself go into the document, and the tool
exits non-zero when this tree's median lies more than that spread above the parent's.

    python tools/bench_json_nullable.py [--steps 20] [--warmup 5] [--copies 100] [--parent-lib PATH] [--out profiles/json_nullable/bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_csv import HBM_PEAK, device_text, measure  # noqa: E402

BID = [("auction", "int32"), ("bidder", "int32"), ("price", "int32"), ("b_date_time", "int64")]
OLD = [(n, t) for n, t in BID]


def bid_block(rows_of, null_col=None, every=False, absent=False):
    """the block's lines; row k (k % 10 == 3) carries the NULLs / lacks `price`.  -> (text, {name: validity of the block's rows})"""
    import numpy as np
    names = [n for n, _ in BID]
    hit = np.arange(len(rows_of)) % 10 == 3
    valid = {n: np.ones(len(rows_of), np.uint8) for n in names}
    out = []
    for k, r in enumerate(rows_of):
        items = list(zip(names, r))
        if hit[k]:
            if absent:
                items = [(n, v) for n, v in items if n != "price"]
                valid["price"][k] = 0
            for j, (n, v) in enumerate(items):
                if every or n == null_col:
                    items[j] = (n, None)
                    valid[n][k] = 0
        out.append(b"{" + b",".join(b'"%s":%s' % (n.encode(), b"null" if v is None else b"%d" % v) for n, v in items) + b"}\n")
    return b"".join(out), valid


def alternate(torch, ctx, parent_path, text, steps, warmup):
    """The guard on the first entry point: flockgpu_json_lines_decode of the parent's library and of this one on the same device text, wall ms per call.
    Every round runs parent (context A), this tree, parent (context B): the parent repeated against itself in the same call.  The spread is the distance
    between the medians of A and B -- what two runs of the SAME code differ by here -- and this tree's median may lie at most that far above the parent's
    median over both (faster is no regression).  All three go through the same raw C call: no Python result objects on either side."""
    from flock_amd import _ffi
    lib = C.CDLL(parent_path)
    lib.flockgpu_ctx_create.argtypes, lib.flockgpu_ctx_create.restype = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)], C.c_int
    lib.flockgpu_ctx_destroy.argtypes, lib.flockgpu_ctx_destroy.restype = [C.c_void_p], None
    sig = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_ffi.JsonField), C.c_int, C.POINTER(_ffi.JsonColumn), C.POINTER(C.c_int64)]
    lib.flockgpu_json_lines_decode.argtypes, lib.flockgpu_json_lines_decode.restype = sig, C.c_int
    kinds = {"int32": _ffi.JSON_INT32, "int64": _ffi.JSON_INT64}
    spec = (_ffi.JsonField * len(OLD))(*[_ffi.JsonField(n.encode(), kinds[t]) for n, t in OLD])
    cols, rows = (_ffi.JsonColumn * len(OLD))(), C.c_int64(0)
    handles = []
    for _ in range(2):
        h = C.c_void_p()
        if lib.flockgpu_ctx_create(ctx.device, None, C.byref(h)) != 0:
            raise RuntimeError("the parent's library gave no context")
        handles.append(h)

    def call(fn, h):
        def one():
            if fn(h, text.data_ptr(), text.numel(), spec, len(OLD), cols, C.byref(rows)) != 0:
                raise RuntimeError("a decode failed")
        return one

    runs = [call(lib.flockgpu_json_lines_decode, handles[0]), call(ctx._lib.flockgpu_json_lines_decode, ctx._h), call(lib.flockgpu_json_lines_decode, handles[1])]
    for _ in range(warmup):
        for run in runs:
            run()
    torch.cuda.synchronize()
    ms = [[], [], []]
    for _ in range(2 * steps):
        for k, run in enumerate(runs):
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    for h in handles:
        lib.flockgpu_ctx_destroy(h)
    med = statistics.median
    pa, ours, pb, parent = med(ms[0]), med(ms[1]), med(ms[2]), med(ms[0] + ms[2])
    spread = abs(pa - pb)
    return {"parent_median_ms": round(parent, 4), "this_median_ms": round(ours, 4), "parent_vs_parent_spread_ms": round(spread, 4),
            "parent_a_median_ms": round(pa, 4), "parent_b_median_ms": round(pb, 4), "inside_spread": ours <= parent + spread, "rounds_each": 2 * steps,
            "rows": int(rows.value)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--copies", type=int, default=100)
    ap.add_argument("--block-events", type=int, default=200_000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "json_nullable", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from flock_amd import GpuContext, NEXMarkSource, Window
    ctx = GpuContext(0)
    g = NEXMarkSource(1, a.block_events, Window.element_wise(), seed=20260926).generate_data(ctx, relations=("bid",))
    cols = {k: getattr(g.bids, k).cpu().numpy() for k, _ in BID}
    rows_of = list(zip(*(cols[k].tolist() for k, _ in BID)))
    n_block, rows = len(rows_of), len(rows_of) * a.copies
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{ctx.device}")
    texts = {"no_nulls": bid_block(rows_of), "null_10pct_one_column": bid_block(rows_of, null_col="price"),
             "null_10pct_every_column": bid_block(rows_of, every=True), "absent_10pct": bid_block(rows_of, absent=True)}
    out = {"rows": rows, "steps": a.steps, "warmup": a.warmup, "hbm_peak_bytes_per_s": HBM_PEAK,
           "note": "fractions of the peak are algorithmic bytes (text read by the pass + what it writes) / the kernel's median duration / 8 TB/s"}

    def check(got, valid, n, want_valid):
        ok = n == rows and sorted(valid) == sorted(k for k, v in want_valid.items() if not v.all())
        for name, _ in BID:
            want = torch.from_numpy(np.where(want_valid[name] == 1, cols[name], 0).astype(cols[name].dtype)).to(got[name].device)
            ok = ok and bool((got[name].reshape(a.copies, n_block) == want).all())
            if name in valid:
                ok = ok and bool((valid[name].reshape(a.copies, n_block) == dev(want_valid[name])).all())
        if not ok:
            raise RuntimeError("the decode differs from the generated columns")

    col_bytes = rows * (4 + 4 + 4 + 8)
    for name, (block, want_valid) in texts.items():
        text = device_text(torch, ctx, b"", block, a.copies)
        check(*ctx.json_lines_decode_nullable(text, BID, borrow=True), want_valid)
        m = measure(torch, ctx, lambda: ctx.json_lines_decode_nullable(text, BID, borrow=True), a.steps, a.warmup)
        m["retry_kernel_ran"] = "json_nparse_retry_kernel" in m["kernels"]
        nb = text.numel()
        for k in ("json_nparse_kernel", "json_nparse_retry_kernel"):
            if k in m["kernels"] and m["kernels"][k]["median_ms"]:
                b = nb + 4 * rows + col_bytes + 4 * rows            # the text, the line index, the columns, four validity bytes per row
                m["kernels"][k]["algorithmic_bytes"] = int(b)
                m["kernels"][k]["frac_of_hbm_peak"] = round(b / (m["kernels"][k]["median_ms"] * 1e-3) / HBM_PEAK, 4)
        m["text_bytes"], m["rows_per_s"] = int(nb), round(rows / (m["wall_ms"]["median"] * 1e-3))
        out["nullable_" + name] = m
        if name == "no_nulls":
            got, n = ctx.json_lines_decode(text, OLD, borrow=True)
            check(got, {}, n, want_valid)
            m = measure(torch, ctx, lambda: ctx.json_lines_decode(text, OLD, borrow=True), a.steps, a.warmup)
            if m["kernels"].get("json_parse_kernel", {}).get("median_ms"):
                b = nb + 4 * rows + col_bytes
                m["kernels"]["json_parse_kernel"]["algorithmic_bytes"] = int(b)
                m["kernels"]["json_parse_kernel"]["frac_of_hbm_peak"] = round(b / (m["kernels"]["json_parse_kernel"]["median_ms"] * 1e-3) / HBM_PEAK, 4)
            m["text_bytes"], m["rows_per_s"] = int(nb), round(rows / (m["wall_ms"]["median"] * 1e-3))
            out["first_decoder_no_nulls"] = m
            if a.parent_lib:
                out["first_decoder_against_parent"] = alternate(torch, ctx, a.parent_lib, text, a.steps, a.warmup)
        del text
    # a Float64 column on the compact path: the bids with `price` written as <price>.50 (two fraction digits, one trailing zero to fold)
    block = b"".join(b'{"auction":%d,"bidder":%d,"price":%d.50,"b_date_time":%d}\n' % r for r in rows_of)
    text = device_text(torch, ctx, b"", block, a.copies)
    ffields = [(n, "float64" if n == "price" else t) for n, t in BID]
    got, valid, n = ctx.json_lines_decode_nullable(text, ffields, borrow=True)
    if n != rows or valid or not bool((got["price"].reshape(a.copies, n_block) == dev(cols["price"].astype(np.float64) + 0.5)).all()):
        raise RuntimeError("the Float64 text does not decode to price + 0.5")
    m = measure(torch, ctx, lambda: ctx.json_lines_decode_nullable(text, ffields, borrow=True), a.steps, a.warmup)
    m["retry_kernel_ran"] = "json_nparse_retry_kernel" in m["kernels"]
    if m["kernels"].get("json_nparse_kernel", {}).get("median_ms"):
        b = text.numel() + 4 * rows + rows * (4 + 4 + 8 + 8) + 4 * rows
        m["kernels"]["json_nparse_kernel"]["algorithmic_bytes"] = int(b)
        m["kernels"]["json_nparse_kernel"]["frac_of_hbm_peak"] = round(b / (m["kernels"]["json_nparse_kernel"]["median_ms"] * 1e-3) / HBM_PEAK, 4)
    m["text_bytes"], m["rows_per_s"] = int(text.numel()), round(rows / (m["wall_ms"]["median"] * 1e-3))
    out["nullable_float64_column"] = m
    del text, got
    # the encoder's own output read back: ten copies' worth of rows with NULLs in 10 % of `price`
    er = n_block * min(a.copies, 10)
    hole = (np.arange(er) % 10 != 3).astype(np.uint8)
    columns = [(n, "timestamp_ms" if n == "b_date_time" else t, dev(np.tile(cols[n], min(a.copies, 10)))) for n, t in BID]
    text = ctx.json_lines_encode(columns, {"price": dev(hole)})
    padded = torch.zeros((text.numel() + 31) // 16 * 16, dtype=torch.uint8, device=text.device)
    padded[: text.numel()] = text
    text = padded[: text.numel()]
    fields = [(n, t) for n, t, _ in columns]
    got, valid, n = ctx.json_lines_decode_nullable(text, fields, borrow=True)
    if n != er or sorted(valid) != ["price"] or not bool((valid["price"] == dev(hole)).all()) or not bool((got["auction"] == columns[0][2]).all()):
        raise RuntimeError("the encoder's text does not read back")
    m = measure(torch, ctx, lambda: ctx.json_lines_decode_nullable(text, fields, borrow=True), a.steps, a.warmup)
    m["rows"], m["text_bytes"], m["rows_per_s"] = er, int(text.numel()), round(er / (m["wall_ms"]["median"] * 1e-3))
    m["retry_kernel_ran"] = "json_nparse_retry_kernel" in m["kernels"]
    out["nullable_encoder_output"] = m
    try:                                        # the host, on a tenth of the rows: json.loads line by line, and Arrow C++'s JSON reader if it is here
        sample = texts["null_10pct_one_column"][0] * max(a.copies // 10, 1)
        t0 = time.perf_counter()
        k = sum(1 for line in sample.splitlines() if json.loads(line) is not None)
        out["json_loads_host"] = {"rows": k, "s": round(time.perf_counter() - t0, 3), "rows_per_s": round(k / (time.perf_counter() - t0))}
        import io
        import pyarrow as pa
        import pyarrow.json as pajson
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            tb = pajson.read_json(io.BytesIO(sample))
            best = min(best or 1e9, time.perf_counter() - t0)
        out["pyarrow_json_host"] = {"rows": tb.num_rows, "best_s": round(best, 4), "rows_per_s": round(tb.num_rows / best), "threads": pa.cpu_count(), "pyarrow": pa.__version__}
    except ImportError:
        out["pyarrow_json_host"] = None
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))
    ctx.close()
    ab = out.get("first_decoder_against_parent")
    if ab and not ab["inside_spread"]:          # the one gate: the first entry point may not have become slower
        sys.exit("bench_json_nullable: flockgpu_json_lines_decode regressed: %.4f ms against the parent's %.4f ms, more than the parent-against-parent spread "
                 "of %.4f ms above it" % (ab["this_median_ms"], ab["parent_median_ms"], ab["parent_vs_parent_spread_ms"]))


if __name__ == "__main__":
    main()
