"""Stage plans across ranks (flockgpu_plan_exchange_retain, StagedRun(comm=...)) on the inputs of bench.py's arch_ops generator: --seconds 30 of NEXMark events
at 1e6 events/s.  Writes profiles/plan_exchange/bench.json (or --out).

Plans:
  q5-pair    q5's first stage pair: Partial COUNT GROUP BY auction -> Hash([auction]) -> FinalPartitioned
  activity   tests/golden/plans/person_activity.json split at its repartition (a union under GROUP BY person, kind; placed by `person`)
Routes, each the median of --executes runs of StagedRun.run (base relations from the host, root batches back to it):
  retain     StagedRun(on_device=True) on one rank: execute_retain + feed_from, the route there was before the exchange
  host       StagedRun(on_device=False): host Arrow at the stage boundary
  xchg-1     StagedRun(comm=...) over one rank
  xchg-2     two thread ranks on device 0 over the `local` transport, each fed its contiguous stripe; the time is the slower rank's
with the per-phase times of flockgpu_comm_phase_read and, from the library's dispatch-bound events, the emit kernel's time and bytes (destination byte
+ every payload column read and written once + the row list where Utf8 or validity columns need it) as a fraction of the 8 TB/s HBM peak.

send-order: the table emit pass alone, on `bid` as four Int64 columns (key auction) striped over 2, 4 and 8 thread ranks, without NULLs (8-byte
columns) and with NULLs in the three value columns (their validity bytes are taken with gather_u8 at the emitted row list): kernel times summed over the ranks.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PLANS = os.path.join(ROOT, "tests", "golden", "plans")
HBM_PEAK_GBS = 8000.0
EMIT = "partition_emit_table_kernel"


def field(name, dt, nullable=True):
    return {"data_type": dt, "dict_id": 0, "dict_is_ordered": False, "name": name, "nullable": nullable}


def scan(fields):
    return {"execution_plan": "memory_exec", "schema": {"fields": fields, "metadata": {}}, "projection": list(range(len(fields)))}


def column(name, index):
    return {"physical_expr": "column", "name": name, "index": index}


def hashed(inp, name, index):
    return {"execution_plan": "coalesce_batches_exec", "target_batch_size": 4096,
            "input": {"execution_plan": "repartition_exec", "input": inp, "partitioning": {"Hash": [[column(name, index)], 8]}}}


def q5_pair():
    """COUNT(*) GROUP BY auction as the planner writes it: Partial -> Hash([auction]) -> FinalPartitioned"""
    bid = [field("auction", "Int32", False)]
    name = "COUNT(UInt8(1))"
    agg = [{"aggregate_expr": "count", "name": name, "data_type": "UInt64", "nullable": True, "expr": {"physical_expr": "literal", "value": {"UInt8": 1}}}]
    group = [[column("auction", 0), "auction"]]
    part = {"execution_plan": "hash_aggregate_exec", "mode": "Partial", "group_expr": group, "aggr_expr": agg, "input": scan(bid),
            "input_schema": {"fields": bid, "metadata": {}}, "schema": {"fields": [bid[0], field(name + "[count]", "UInt64")], "metadata": {}}}
    return {"execution_plan": "hash_aggregate_exec", "mode": "FinalPartitioned", "group_expr": group, "aggr_expr": agg, "input": hashed(part, "auction", 0),
            "input_schema": {"fields": bid, "metadata": {}}, "schema": {"fields": [bid[0], field(name, "UInt64")], "metadata": {}}}


def summary(times):
    return {"ms_median": round(statistics.median(times), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4), "ms_all": [round(t, 4) for t in times]}


def rate(ms, nbytes):
    return {"ms": round(ms, 4), "bytes": int(nbytes), "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1), "frac_of_hbm_peak": round(nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}


def stripe(rb, r, world):
    lo, hi = rb.num_rows * r // world, rb.num_rows * (r + 1) // world
    return rb.slice(lo, hi - lo)


def on_ranks(world, body):
    """body(rank, gpu, comm, barrier) on `world` threads, each with its own GpuContext (own stream) on device 0"""
    from flock_amd import Comm, GpuContext
    comms = Comm.local(world)
    gpus = [GpuContext(0, own_stream=True) for _ in range(world)]
    barrier = threading.Barrier(world)
    out, err = [None] * world, [None] * world

    def run(r):
        try:
            out[r] = body(r, gpus[r], comms[r], barrier)
        except BaseException as e:   # noqa: BLE001
            err[r] = e
            barrier.abort()
    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    if any(t.is_alive() for t in threads):
        raise RuntimeError("a rank is stuck")
    for e in err:
        if e is not None and not isinstance(e, threading.BrokenBarrierError):
            raise e
    for e in err:
        if e is not None:
            raise e
    for c in comms:
        c.close()
    for g in gpus:
        g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=30)
    ap.add_argument("--eps", type=int, default=1_000_000)
    ap.add_argument("--executes", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_exchange", "bench.json"))
    a = ap.parse_args()
    import numpy as np
    import pyarrow as pa
    from flock_amd import GpuContext, NEXMarkSource, Window
    from flock_amd.runtime import ExecutionContext
    from flock_amd.stages import StagedRun, split_at_repartitions

    gpu = GpuContext(0)
    g = NEXMarkSource(a.seconds, a.eps, Window.element_wise(), seed=11).generate_data(gpu, relations=("bid",))
    b = g.bids
    auction, bidder, price, when = (x.cpu().numpy() for x in (b.auction, b.bidder, b.price, b.b_date_time))
    del g, b
    n = len(price)
    bid_rb = pa.record_batch([pa.array(auction), pa.array(bidder), pa.array(price), pa.array(when).cast(pa.timestamp("ms"))], names=["auction", "bidder", "price", "b_date_time"])
    na = n // 46
    auction_rb = pa.record_batch([pa.array(when[::46][:na]).cast(pa.timestamp("ms")), pa.array(bidder[::46][:na])], names=["a_date_time", "seller"])
    out = {"input": {"bids": n, "auctions": na, "seconds": a.seconds, "eps": a.eps}, "executes": a.executes,
           "recipe": "three untimed runs, then timed runs of StagedRun.run (feed the stripe, every stage, root batches to the host, clean); ranks start a run "
                     "together (a barrier) and the run's time is the slower rank's; phases and kernel events over two further runs"}

    def rows_of(batches):
        return sum(rb.num_rows for rb in batches if rb is not None)

    def one_rank(stages, relations, **mode):
        run = StagedRun(gpu, stages, **mode)
        try:
            rows = rows_of(run.run(relations))
            for _ in range(2):
                run.run(relations)
            gpu.synchronize()
            times = []
            for _ in range(a.executes):
                t0 = time.perf_counter()
                run.run(relations)
                gpu.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
        finally:
            run.close()
        return dict(summary(times), rows=rows)

    def exchange(stages, relations, world, row_bytes):
        def body(r, gp, comm, barrier):
            mine = {k: stripe(rb, r, world) for k, rb in relations.items()}
            run = StagedRun(gp, stages, comm=comm)
            try:
                rows = 0
                for _ in range(3):
                    rows = rows_of(run.run(mine))
                times = []
                for _ in range(a.executes):
                    barrier.wait(timeout=300)
                    t0 = time.perf_counter()
                    run.run(mine)
                    gp.synchronize()
                    barrier.wait(timeout=300)
                    times.append((time.perf_counter() - t0) * 1e3)
                comm.phases(True)
                gp.profile_reset()
                gp.profile_only(None)
                gp.profile(True)
                sent = 0
                for _ in range(2):
                    barrier.wait(timeout=300)
                    run.run(mine)
                    gp.synchronize()
                stats = gp.profile_read()
                gp.profile(False)
                phases = comm.phase_times()
                comm.phases(False)
                sent = 0
                if world > 1:     # rows this rank's first stage produces: its send rows
                    run.ctxs[0].feed_data_sources([[[rb]] for rb in mine.values()])
                    sent = run.ctxs[0].plans[0].execute_retain()
                    run.ctxs[0].clean_data_sources()
            finally:
                run.close()
            return rows, times, stats, phases, sent
        res = on_ranks(world, body)
        e = dict(summary([max(ts) for ts in zip(*[r[1] for r in res])]), rows=sum(r[0] for r in res), ranks=world)
        e["phases_ms_per_run"] = [{k: round(v["total_ms"] / 2, 4) for k, v in r[3].items()} for r in res]
        emit_ms = sum(r[2].get(EMIT, {}).get("total_ms", 0.0) for r in res) / 2
        if emit_ms > 0:
            e["emit_kernel"] = dict(rate(emit_ms, row_bytes * sum(r[4] for r in res)), rows=sum(r[4] for r in res), note="time summed over the ranks (they share one device)")
        e["kernels_ms_per_run_rank0"] = {k: round(v["total_ms"] / 2, 4) for k, v in sorted(res[0][2].items(), key=lambda kv: -kv[1]["total_ms"])[:10]}
        return e

    def run(key, fn):
        try:
            e = fn()
        except Exception as ex:   # (a workload that fails is reported, the others still run)
            e = {"error": repr(ex)}
        out[key] = e
        print(key, json.dumps(e), flush=True)

    act = json.load(open(os.path.join(PLANS, "person_activity.json")))
    workloads = {
        # bytes per send row: destination byte + (4 + 8) read and written
        "q5-pair": (split_at_repartitions(q5_pair()), {"bid": bid_rb.select(["auction"])}, 1 + 2 * (4 + 8)),
        # person Int32, kind Utf8 (row list: 4), COUNT state UInt64
        "activity": (split_at_repartitions(act), {"auction": auction_rb, "bid": bid_rb}, 1 + 2 * (4 + 8) + 4),
    }
    for name, (stages, relations, row_bytes) in workloads.items():
        run(name + "/retain", lambda: one_rank(copy.deepcopy(stages), relations, on_device=True))
        run(name + "/host", lambda: one_rank(copy.deepcopy(stages), relations, on_device=False))
        run(name + "/xchg-1", lambda: exchange(copy.deepcopy(stages), relations, 1, row_bytes))
        run(name + "/xchg-2", lambda: exchange(copy.deepcopy(stages), relations, 2, row_bytes))
        rows = {out[name + k].get("rows") for k in ("/retain", "/host", "/xchg-1", "/xchg-2")}
        if len(rows) != 1:
            out[name + "/rows_differ"] = {"error": "the routes return different row counts: %r" % sorted(rows, key=repr)}

    # ---- send order: the emit pass alone
    cols4 = [field("k", "Int64"), field("a", "Int64"), field("b", "Int64"), field("c", "Int64")]
    plan4 = hashed(scan(cols4), "k", 0)
    vals = [auction.astype(np.int64), price.astype(np.int64), bidder.astype(np.int64), when.astype(np.int64)]
    null = np.random.default_rng(5).random(n) < 0.1

    def send_order(world, with_nulls):
        def body(r, gp, comm, barrier):
            lo, hi = n * r // world, n * (r + 1) // world
            arrs = [pa.array(v[lo:hi], mask=(null[lo:hi] if with_nulls and i else None)) for i, v in enumerate(vals)]
            ctx = ExecutionContext([plan4], gpu=gp, generic_only=True)
            try:
                ctx.feed_data_sources([[[pa.record_batch(arrs, names=["k", "a", "b", "c"])]]])
                for _ in range(3):
                    ctx.exchange_retain(comm)
                gp.profile_reset()
                gp.profile_only(None)
                gp.profile(True)
                for _ in range(3):
                    barrier.wait(timeout=300)
                    ctx.exchange_retain(comm)
                    gp.synchronize()
                stats = gp.profile_read()
                gp.profile(False)
                ctx.clean_data_sources()
            finally:
                ctx.close()
            return stats
        res = on_ranks(world, body)
        tot = {}
        for st in res:
            for k, v in st.items():
                if k.startswith(("partition_", "gather_")):
                    tot[k] = tot.get(k, 0.0) + v["total_ms"] / 3
        row_bytes = 1 + 2 * 8 * 4 + (4 if with_nulls else 0)      # destination byte, four Int64 read and written, the row list the validity take reads
        e = {"ranks": world, "rows": n, "kernels_ms_per_call_all_ranks": {k: round(v, 4) for k, v in sorted(tot.items())}}
        if tot.get(EMIT):
            e["emit_kernel"] = rate(tot[EMIT], row_bytes * n)
        return e
    for world in (2, 4, 8):
        run("send-order/int64x4/%d" % world, lambda: send_order(world, False))
        run("send-order/int64x4+validity/%d" % world, lambda: send_order(world, True))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) else v.get("ms_median", v.get("error", v.get("emit_kernel")))) for k, v in out.items() if k != "input"}))
    gpu.close()
    if any(isinstance(v, dict) and "error" in v for v in out.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
