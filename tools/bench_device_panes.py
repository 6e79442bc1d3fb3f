"""Panes of the window ring from device columns (flockgpu_plan_feed_pane_columns) and the event-time pane split (flockgpu_pane_split), in one process.

Readings, every result compared with the host route before anything is timed; 5 warm-up and 20 timed calls, medians:
  q5_per_window      q5 Hopping(10, 5) at --eps events/s: one window = feed the new pane, execute, clean.  Three routes: the pane fed from device columns
                     (`device_ring`), from registered host memory with flockgpu_plan_feed_pane (`host_ring`, the parent's only route into a ring), and no
                     ring at all: both panes of the window re-fed whole with flockgpu_plan_feed_columns (`device_whole`);
  rows_ring_per_window  the same three routes for q7's plan, whose ring keeps the panes' rows;
  split_ordered      flockgpu_pane_split over the b_date_time column of --seconds s of bids generated on the device (time-ordered: no row list): the whole
                     call, and the streaming pass as a fraction of the 8 TB/s peak (ALGORITHMIC bytes, 8 a row; no counter was read) -- next to
                     flockgpu_memcpy of the same column and the library's q7_max_kernel over the price column (VERDICT.md's read-only ceiling), same run;
  split_unordered    the same timestamps with each pane's rows shuffled across two panes (the row-list route): the whole call;
  end_to_end         serde_json lines -> decode -> pane split -> ring -> execute -> result columns -> CSV, pane by pane, nothing on the host: the whole call;
  against_parent     (--parent-lib: a libflockgpu.so built from the parent commit) the two entry points whose bodies were factored out: the copying
                     flockgpu_plan_feed_columns of tools/bench_device_feed.py and flockgpu_plan_feed_pane from registered memory; parent, this tree, parent
                     again per round through the same raw C calls.  The margin is the spread between the parent's own two medians; the tool exits
                     non-zero when this tree's median lies further above the parent's.
Writes one JSON document (default profiles/device_panes/bench.json) and prints it.

    python tools/bench_device_panes.py [--seconds 100] [--eps 1000000] [--steps 20] [--warmup 5] [--parent-lib PATH] [--out profiles/device_panes/bench.json]"""
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
from bench_csv import HBM_PEAK, measure  # noqa: E402
from bench_device_feed import BID, bid_filter_plan  # noqa: E402

HOP_MS, PPW = 5_000, 2


def rows_of(rb):
    return sorted(zip(*[c.to_pylist() for c in rb.columns]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=100)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--text-seconds", type=int, default=30)
    ap.add_argument("--text-eps", type=int, default=200_000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_panes", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    import torch
    from flock_amd import GpuContext, NEXMarkSource, Window, WindowSchedule, _ffi
    from flock_amd.nexmark import NEXMARK_JSON_SCHEMAS, columns_to_event_bytes, event_source
    from flock_amd.runtime import ExecutionContext, _exported, device_panes
    gpu = GpuContext(0)
    lib = _ffi.load()
    g = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid",))
    columns, _ = event_source("bid", g.bids)
    rows = columns[0][2].numel()
    t_col = g.bids.b_date_time
    origin = int(t_col[0])
    out = {"input": {"bids": rows, "seconds": a.seconds, "eps": a.eps, "hop_ms": HOP_MS, "panes_per_window": PPW}, "steps": a.steps, "warmup": a.warmup,
           "hbm_peak_bytes_per_s": HBM_PEAK,
           "recipe": "wall medians of `steps` calls after `warmup`, each call ending in a synchronise; kernels from the library's dispatch-bound events over the same "
                     "calls again; fractions of the peak are algorithmic bytes / the kernel's median duration / 8 TB/s"}

    # ---- the pane split, ordered path: checked against numpy, then timed next to a copy of the column and the library's read-only pass
    first, bounds, row_list = gpu.pane_split(t_col, HOP_MS, origin)
    ids = torch.div(t_col - origin, HOP_MS, rounding_mode="floor")
    want = torch.searchsorted(ids, torch.arange(int(ids[0]), int(ids[-1]) + 2, device=ids.device)).cpu().numpy()
    if row_list is not None or first != int(ids[0]) or bounds.tolist() != want.tolist():
        raise RuntimeError("split_ordered: the bounds differ from searchsorted's")
    n_panes = len(bounds) - 1
    m = measure(torch, gpu, lambda: gpu.pane_split(t_col, HOP_MS, origin), a.steps, a.warmup)
    k = m["kernels"].get("pane_census_kernel", {})
    if k.get("median_ms"):
        k["algorithmic_bytes"], k["frac_of_hbm_peak"] = rows * 8, round(rows * 8 / (k["median_ms"] * 1e-3) / HBM_PEAK, 4)
    m["panes"], m["rows_per_s"] = n_panes, round(rows / (m["wall_ms"]["median"] * 1e-3))
    out["split_ordered"] = m
    twin = torch.empty_like(t_col)
    m = measure(torch, gpu, lambda: gpu._check(lib.flockgpu_memcpy(gpu._h, twin.data_ptr(), t_col.data_ptr(), rows * 8, _ffi.D2D)), a.steps, a.warmup)
    m["hbm_GBps_read_plus_written"] = round(2 * rows * 8 / (m["wall_ms"]["median"] * 1e-3) / 1e9, 1)
    out["memcpy_same_column"] = m
    del twin
    whole = WindowSchedule.single(rows)
    m = measure(torch, gpu, lambda: gpu.q7_highest_bid(g.bids, whole), a.steps, a.warmup)
    k = m["kernels"].get("q7_max_kernel", {})
    if k.get("median_ms"):
        k["algorithmic_bytes"], k["frac_of_hbm_peak"] = rows * 4, round(rows * 4 / (k["median_ms"] * 1e-3) / HBM_PEAK, 4)
    out["q7_max_kernel_same_rows"] = {"kernels": {"q7_max_kernel": k}}

    # ---- the unordered path: each pane's rows shuffled across two panes
    torch.manual_seed(7)
    idx = torch.arange(rows, device=t_col.device)
    for j in range(0, n_panes - 1, 2):
        lo, hi = int(bounds[j]), int(bounds[j + 2])
        idx[lo:hi] = lo + torch.randperm(hi - lo, device=t_col.device)
    t_mixed = t_col[idx].contiguous()
    f2, b2, r2 = gpu.pane_split(t_mixed, HOP_MS, origin)
    ids2 = torch.div(t_mixed - origin, HOP_MS, rounding_mode="floor")
    if r2 is None or f2 != first or b2.tolist() != bounds.tolist():
        raise RuntimeError("split_unordered: the bounds differ from the ordered column's")
    r2l = r2.to(torch.int64)
    if not bool(((ids2[r2l][1:] > ids2[r2l][:-1]) | ((ids2[r2l][1:] == ids2[r2l][:-1]) & (r2l[1:] > r2l[:-1]))).all()):
        raise RuntimeError("split_unordered: the row list is not a stable grouping")
    m = measure(torch, gpu, lambda: gpu.pane_split(t_mixed, HOP_MS, origin), a.steps, a.warmup)
    m["rows_per_s"] = round(rows / (m["wall_ms"]["median"] * 1e-3))
    out["split_unordered"] = m
    del idx, t_mixed, ids2, r2, r2l, ids

    # ---- per window, three routes; the panes are the split's
    panes = [(p, c, v) for p, c, v in device_panes(gpu, columns, {}, "b_date_time", HOP_MS, origin)][:8]
    P = len(panes)
    host = [{name: col.cpu().numpy() for name, _, col in c} for _, c, _ in panes]
    regs = [arr.ctypes.data for h in host for arr in h.values() if lib.flockgpu_host_register(C.c_void_p(arr.ctypes.data), arr.nbytes) == 0]
    batches = [pa.record_batch([pa.array(h[n]).cast(pa.timestamp("ms")) if n == "b_date_time" else pa.array(h[n]) for n, _ in BID], names=[n for n, _ in BID]) for h in host]

    def routes(plan_text, generic_only=False):
        ring_d = ExecutionContext([plan_text], gpu=gpu, generic_only=generic_only)
        ring_h = ExecutionContext([plan_text], gpu=gpu, generic_only=generic_only)
        flat = ExecutionContext([plan_text], gpu=gpu, generic_only=generic_only)
        ring_d.open_window_ring(PPW)
        ring_h.open_window_ring(PPW)
        at = {"d": 0, "h": 0, "w": 1}
        last = {}

        def device_ring():
            k = at["d"]
            ring_d.feed_device_sources([(panes[k % P][1], panes[k % P][2])], pane=k)
            last["d"] = ring_d.execute()[0][0]
            ring_d.clean_data_sources()
            at["d"] = k + 1

        def host_ring():
            k = at["h"]
            ring_h.feed_data_sources([[[batches[k % P]]]], pane=k)
            last["h"] = ring_h.execute()[0][0]
            ring_h.clean_data_sources()
            at["h"] = k + 1

        def device_whole():
            k = at["w"]
            for q in range(k - PPW + 1, k + 1):
                flat.plans[0].feed_columns(0, panes[q % P][1], panes[q % P][2])
            last["w"] = flat.execute()[0][0]
            flat.clean_data_sources()
            at["w"] = k + 1

        device_ring()
        host_ring()
        for _ in range(P):                                  # every window of one lap, the three routes side by side
            device_ring()
            host_ring()
            device_whole()
            if not (rows_of(last["d"]) == rows_of(last["h"]) == rows_of(last["w"])):
                raise RuntimeError("the three routes differ at window %d" % (at["d"] - 1))
        res = {"rows_per_pane": int(panes[0][1][0][2].numel()), "query": ring_d.plans[0].query}
        for name, call in (("device_ring", device_ring), ("host_ring", host_ring), ("device_whole", device_whole)):
            res[name] = measure(torch, gpu, call, a.steps, a.warmup)
        for c in (ring_d, ring_h, flat):
            c.close()
        return res

    plans = os.path.join(ROOT, "tests", "golden", "plans")
    out["q5_per_window"] = routes(open(os.path.join(plans, "q5.json")).read())
    out["rows_ring_per_window"] = routes(open(os.path.join(plans, "q7.json")).read())

    # ---- the two refactored entry points against the parent commit's library
    if a.parent_lib:
        out["against_parent"] = against_parent(a, gpu, torch, lib, columns, rows, batches, _exported, os.path.join(plans, "q5.json"))
    for ptr in regs:
        lib.flockgpu_host_unregister(C.c_void_p(ptr))
    del panes, host, batches, columns, g

    # ---- text in, text out
    block = NEXMarkSource(a.text_seconds, a.text_eps, Window.element_wise(), seed=12).generate_data(gpu, relations=("bid",)).bids
    bids = {k: getattr(block, k) for k in ("auction", "bidder", "price", "b_date_time")}
    text = columns_to_event_bytes(gpu, "bid", bids)
    n_text, t0 = bids["auction"].numel(), int(bids["b_date_time"][0])
    e2e = ExecutionContext([open(os.path.join(plans, "q5.json")).read()], gpu=gpu)
    ref = ExecutionContext([open(os.path.join(plans, "q5.json")).read()], gpu=gpu)
    e2e.open_window_ring(PPW)
    state = {"origin": t0, "texts": [], "panes": 0}

    def end_to_end():
        cols, n = gpu.json_lines_decode(text, NEXMARK_JSON_SCHEMAS["bid"])
        src_cols, src_valid = event_source("bid", cols)
        texts = []
        for p, c, v in device_panes(gpu, src_cols, src_valid, "b_date_time", HOP_MS, state["origin"]):
            e2e.feed_device_sources([(c, v)], pane=p)
            e2e.execute_retain()
            texts.append(gpu.csv_encode(*e2e.result_columns()[:2]))
            e2e.clean_data_sources()
        gpu.synchronize()
        state["origin"] -= len(texts) * HOP_MS            # (the next call's panes follow this call's in the ring)
        state["texts"], state["panes"] = texts, len(texts)
    end_to_end()
    hb = {k: v.cpu().numpy() for k, v in bids.items()}
    cut = np.searchsorted(np.floor_divide(hb["b_date_time"] - t0, HOP_MS), np.arange(state["panes"] + 1))
    ref.open_window_ring(PPW)
    for p in range(state["panes"]):
        lo, hi = int(cut[p]), int(cut[p + 1])
        rb = pa.record_batch([pa.array(hb[n][lo:hi]).cast(pa.timestamp("ms")) if n == "b_date_time" else pa.array(hb[n][lo:hi]) for n, _ in BID], names=[n for n, _ in BID])
        ref.feed_data_sources([[[rb]]], pane=p)
        want = rows_of(ref.execute()[0][0])
        ref.clean_data_sources()
        lines = bytes(state["texts"][p].cpu().numpy()).decode().splitlines()[1:]
        if sorted(tuple(int(x) for x in line.split(",")) for line in lines) != want:
            raise RuntimeError("end_to_end: window %d differs from the host route" % p)
    m = measure(torch, gpu, end_to_end, a.steps, a.warmup)
    m.update({"rows_in": n_text, "json_bytes_in": int(text.numel()), "panes": state["panes"], "rows_per_s": round(n_text / (m["wall_ms"]["median"] * 1e-3), 1)})
    out["end_to_end"] = m
    e2e.close()
    ref.close()
    gpu.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    bad = [k for k, v in out.get("against_parent", {}).items() if not v["inside_spread"]]
    if bad:
        sys.exit("bench_device_panes: slower than the parent commit beyond the parent-against-parent spread: " + ", ".join(bad))


def against_parent(a, gpu, torch, lib, columns, rows, batches, exported, q5_path):
    """parent (context A), this tree, parent (context B) per round, through the same raw C calls; medians of 2 x steps rounds"""
    from flock_amd import _ffi
    parent = C.CDLL(a.parent_lib)
    for name in ("flockgpu_ctx_create", "flockgpu_ctx_destroy", "flockgpu_ctx_synchronize", "flockgpu_plan_create_ex", "flockgpu_plan_destroy", "flockgpu_plan_reset",
                 "flockgpu_plan_feed_columns", "flockgpu_plan_ring_open", "flockgpu_plan_feed_pane"):
        getattr(parent, name).restype, getattr(parent, name).argtypes = _ffi.SYMBOLS[name]
    spec, n_rows, keep = gpu._text_columns(columns, None)
    threshold = 1 << 30
    texts = {"copy_feed": json.dumps(bid_filter_plan(threshold)).encode(), "feed_pane_registered": open(q5_path).read().encode()}
    res = {}
    for what, plan_text in texts.items():
        sides = []
        for which in (parent, lib, parent):
            h, p = C.c_void_p(), C.c_void_p()
            if which.flockgpu_ctx_create(gpu.device, None, C.byref(h)) != 0 or which.flockgpu_plan_create_ex(h, plan_text, len(plan_text), 0, C.byref(p)) != 0:
                raise RuntimeError("against_parent: no context / plan")
            if what == "feed_pane_registered" and which.flockgpu_plan_ring_open(p, PPW) != 0:
                raise RuntimeError("against_parent: ring_open failed")
            sides.append({"lib": which, "h": h, "p": p, "k": 0})

        def call(s):
            if what == "copy_feed":
                rc = s["lib"].flockgpu_plan_reset(s["p"]) or s["lib"].flockgpu_plan_feed_columns(s["p"], 0, spec, len(columns), n_rows, 0)
            else:
                with exported([batches[s["k"] % len(batches)]]) as (schema, ptrs):
                    rc = s["lib"].flockgpu_plan_feed_pane(s["p"], 0, s["k"], schema, ptrs, 1)
                    rc = rc or s["lib"].flockgpu_ctx_synchronize(s["h"])
                rc = rc or s["lib"].flockgpu_plan_reset(s["p"])
                s["k"] += 1
            rc = rc or s["lib"].flockgpu_ctx_synchronize(s["h"])
            if rc != 0:
                raise RuntimeError("against_parent: %s failed with %d" % (what, rc))
        for _ in range(a.warmup):
            for s in sides:
                call(s)
        torch.cuda.synchronize()
        ms = [[], [], []]
        for _ in range(2 * a.steps):
            for i, s in enumerate(sides):
                t0 = time.perf_counter()
                call(s)
                ms[i].append((time.perf_counter() - t0) * 1e3)
        for s in sides:
            s["lib"].flockgpu_plan_destroy(s["p"])
            s["lib"].flockgpu_ctx_destroy(s["h"])
        med = statistics.median
        pa_, ours, pb, both = med(ms[0]), med(ms[1]), med(ms[2]), med(ms[0] + ms[2])
        spread = abs(pa_ - pb)
        res[what] = {"parent_median_ms": round(both, 4), "this_median_ms": round(ours, 4), "parent_vs_parent_spread_ms": round(spread, 4),
                     "parent_a_median_ms": round(pa_, 4), "parent_b_median_ms": round(pb, 4), "inside_spread": ours <= both + spread, "rounds_each": 2 * a.steps}
    return res


if __name__ == "__main__":
    main()
