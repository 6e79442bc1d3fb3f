"""Stage DAGs through `StagedRun(gpu, stages, comm=...)`: every rank (a thread with its own stream on device 0, `local` transport) runs the same
stages over its contiguous stripe of the base relations, hands every stage's result over with flockgpu_plan_exchange_retain and reads it with
flockgpu_plan_feed_from.  The union of the ranks' root batches must be the whole plan executed on one context, as a multiset -- and the CPU
interpreter's rows where tests/plan_interp.py takes the plan."""
import json
import os

import numpy as np
import pyarrow as pa
import pytest

import plan_corpus as pc
import plan_interp as pi
from test_gpu_plan_exchange import multiset, rows_of, run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")
TS = pa.timestamp("ms")
WORLDS = [1, 2, 3]


def _golden(name):
    return json.load(open(os.path.join(PLANS, name + ".json")))


def _stripe(rb, r, world):
    lo, hi = rb.num_rows * r // world, rb.num_rows * (r + 1) // world
    return rb.slice(lo, hi - lo)


def _whole(plan, relations):
    from flock_amd import GpuContext
    from flock_amd.runtime import ExecutionContext, collect
    gpu = GpuContext(0)
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        return rows_of(collect(ctx, [[[rb]] for rb in relations.values()])[0])
    finally:
        ctx.close()
        gpu.close()


def _interp(plan, relations):
    """the interpreter's rows over the same relations (columns a leaf names and the relation lacks are NULL), or None where it does not take the plan"""
    tables = []
    for fields in pi.leaf_schemas(plan):
        names = {f["name"] for f in fields}
        rb = next(rb for rb in relations.values() if set(rb.schema.names) <= names)
        cols = {n: (rb[n].cast(pa.int64()) if pa.types.is_timestamp(rb[n].type) else rb[n]).to_pylist() for n in rb.schema.names}
        tables.append({f["name"]: cols.get(f["name"], [None] * rb.num_rows) for f in fields})
    try:
        return rows_of_py(pi.run_plan(plan, tables)[2])
    except NotImplementedError:
        return None


def rows_of_py(rows):
    import struct
    return [tuple(("f", struct.unpack("<q", struct.pack("<d", v))[0]) if isinstance(v, float) else v for v in r) for r in rows]


def _staged(world, stages, relations):
    from flock_amd.stages import StagedRun

    def body(r, gpu, comm):
        run = StagedRun(gpu, stages, comm=comm)
        try:
            mine = {k: _stripe(rb, r, world) for k, rb in relations.items()}
            first = rows_of(run.run(mine))
            again = rows_of(run.run(mine))                  # the plans are reusable: a second window through the same instances
            assert multiset(again) == multiset(first)       # (a hash aggregate's groups and a join's pairs come in no defined order)
            return first
        finally:
            run.close()
    return run_ranks(world, body)


def _check(world, plan, stages, relations, ordered=False):
    want = _whole(plan, relations)
    assert want, "the case is vacuous"
    per_rank = _staged(world, stages, relations)
    got = [row for g in per_rank for row in g]
    if ordered:
        assert per_rank[0] == want and all(g == [] for g in per_rank[1:])
    assert multiset(got) == multiset(want)
    ref = _interp(plan, relations)
    if ref is not None:
        assert multiset(ref) == multiset(want)
    return per_rank


# ------------------------------------------------------------------ relations
def _nexmark(seed, eps, n):
    from test_stage_plans import _relations
    return _relations(seed, eps, n)[0]


def _c123(n, seed):
    r = np.random.default_rng(seed)
    c3 = [pc.word(x) for x in r.integers(0, 60, n)]
    return {"t": pa.record_batch([pa.array(r.integers(-50, 50, n)), pa.array(r.integers(-800, 800, n) / 4.0), pa.array(c3, pa.string())], names=["c1", "c2", "c3"])}


@pytest.mark.parametrize("world", WORLDS)
def test_q3_both_sides_hash_partitioned_with_utf8_payload(world):
    from flock_amd.stages import build_query_dag
    rel = _nexmark(3, 50_000, 150_000)
    plan = _golden("q3")
    _check(world, plan, build_query_dag(plan), {"auction": rel["auction"], "person": rel["person"]})


@pytest.mark.parametrize("world", WORLDS)
def test_partial_hash_final_with_a_utf8_key(world):
    from flock_amd.stages import build_query_dag
    plan = _golden("golden_aggregate")
    per_rank = _check(world, plan, build_query_dag(plan), _c123(5000, 1))
    if world > 1:
        assert sum(1 for g in per_rank if g) > 1          # the groups are spread over the ranks


@pytest.mark.parametrize("world", WORLDS)
def test_q17_composite_key_placed_by_its_first_column(world):
    from flock_amd.stages import split_at_repartitions
    bid = _nexmark(17, 20_000, 20_000)["bid"]
    assert bid.num_rows >= 2 * 8192 + 3
    plan = _golden("q17_auction_stats")
    _check(world, plan, split_at_repartitions(plan), {"bid": bid.slice(0, 2 * 8192 + 3)})


@pytest.mark.parametrize("world", WORLDS)
def test_person_activity_a_union_under_group_by(world):
    from flock_amd.stages import split_at_repartitions
    bid = _nexmark(21, 20_000, 6_000)["bid"]
    na = bid.num_rows // 7
    auction = pa.record_batch([bid["b_date_time"].slice(0, na), bid["bidder"].slice(0, na)], names=["a_date_time", "seller"])
    plan = _golden("person_activity")
    _check(world, plan, split_at_repartitions(plan), {"auction": auction, "bid": bid})


@pytest.mark.parametrize("world", WORLDS)
def test_a_semi_join_whose_two_inputs_are_hash_partitioned(world):
    from flock_amd.stages import build_query_dag
    left = pc.scan([("l_k", "Int32"), ("l_s", "Utf8"), ("l_id", "Int64")])
    right = pc.scan([("r_k", "Int32"), ("r_v", "Int64")])
    plan = pc.join("Semi", left, right, [("l_k", "r_k")]).plan
    r = np.random.default_rng(2)
    nl, nr = 4000, 700
    lk = pc.with_nulls([int(x) for x in r.integers(0, 3000, nl)], 0.1, r)
    rk = pc.with_nulls([int(x) for x in r.integers(0, 3000, nr)], 0.1, r)
    rel = {"l": pa.record_batch([pa.array(lk, pa.int32()), pa.array(pc.with_nulls([pc.word(x) for x in r.integers(0, 90, nl)], 0.2, r), pa.string()),
                                 pa.array(list(range(nl)), pa.int64())], names=["l_k", "l_s", "l_id"]),
           "r": pa.record_batch([pa.array(rk, pa.int32()), pa.array([int(x) for x in r.integers(-9, 9, nr)], pa.int64())], names=["r_k", "r_v"])}
    _check(world, plan, build_query_dag(plan), rel)


@pytest.mark.parametrize("world", WORLDS)
def test_a_sort_above_a_gather_edge_runs_on_rank_zero_in_order(world):
    from flock_amd.stages import build_query_dag, distributed_placement
    plan = _golden("golden_aggregate_sorted")
    stages = build_query_dag(plan)
    assert distributed_placement(stages) == (["key", "gather", "gather"], ["all", "all", "zero"])
    _check(world, plan, stages, _c123(5000, 4), ordered=True)


def test_a_broadcast_edge_is_refused_by_name():
    """a one-row side (a global MAX: gathered) joined against a partitioned side -- q5's `num = maxn` join on the generic operators"""
    from flock_amd import Comm, GpuContext
    from flock_amd.stages import Stage, StagedRun
    counts = pc.scan([("k", "Int32"), ("num", "Int64")])
    side = pc.scan([("m", "Int64")])
    mx = pc.aggregate(side, [], [("max", "m")], single="Partial")
    join = {"execution_plan": "hash_join_exec", "left": pc.scan(counts.cols).plan, "right": pc.scan(mx.cols).plan, "join_type": "Inner", "mode": "Partitioned",
            "on": [[counts.c("num"), pc.col(mx.cols[0][0], mx.cols)]], "schema": pc.schema(counts.cols + mx.cols)}
    stages = [Stage(pc.hashed(counts, "k"), [None]), Stage(mx.plan, [None]), Stage(join, [0, 1])]
    comm, gpu = Comm.local(1)[0], GpuContext(0, own_stream=True)
    try:
        with pytest.raises(NotImplementedError) as e:
            StagedRun(gpu, stages, comm=comm)
        assert "broadcast edge" in str(e.value) and "stage 1 -> stage 2" in str(e.value)
        StagedRun(gpu, stages, on_device=True).close()        # the other modes take the same stages
    finally:
        comm.close()
        gpu.close()
