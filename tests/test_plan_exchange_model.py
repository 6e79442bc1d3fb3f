"""CPU side of the plan exchange (flockgpu_plan_exchange_retain, `StagedRun(comm=...)`):
  1. the stage DAGs of tests/test_gpu_staged_exchange.py, run stage by stage over tests/plan_exchange_model.py with the CPU interpreter as the
     executor, give the whole plan's rows at every world size -- the cut, the placement by the first hash column and the gather edges are sound;
  2. the header declares the entry and the built library exports it;
  3. the Python surface lists it, and StagedRun takes a communicator."""
import ctypes
import inspect
import json
import os
import re

import pyarrow as pa
import pytest

import plan_corpus as pc
import plan_exchange_model as model
import plan_interp as pi
from test_gpu_plan_exchange import multiset
from test_gpu_staged_exchange import _c123, _golden, _nexmark, rows_of_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(rb):
    return {n: (rb[n].cast(pa.int64()) if pa.types.is_timestamp(rb[n].type) else rb[n]).to_pylist() for n in rb.schema.names}


def _cases():
    from flock_amd.stages import build_query_dag, split_at_repartitions
    rel = _nexmark(3, 50_000, 60_000)
    yield "q3", _golden("q3"), build_query_dag, {"auction": rel["auction"], "person": rel["person"]}
    yield "golden_aggregate", _golden("golden_aggregate"), build_query_dag, _c123(1500, 1)
    yield "golden_aggregate_sorted", _golden("golden_aggregate_sorted"), build_query_dag, _c123(1500, 4)
    bid = _nexmark(17, 20_000, 4_000)["bid"]
    yield "q17_auction_stats", _golden("q17_auction_stats"), split_at_repartitions, {"bid": bid}
    na = bid.num_rows // 7
    auction = pa.record_batch([bid["b_date_time"].slice(0, na), bid["bidder"].slice(0, na)], names=["a_date_time", "seller"])
    yield "person_activity", _golden("person_activity"), split_at_repartitions, {"auction": auction, "bid": bid}
    left = pc.scan([("l_k", "Int32"), ("l_id", "Int64")])
    right = pc.scan([("r_k", "Int32"), ("r_v", "Int64")])
    semi = {"l": pa.record_batch([pa.array([i % 97 if i % 11 else None for i in range(900)], pa.int32()), pa.array(list(range(900)), pa.int64())], names=["l_k", "l_id"]),
            "r": pa.record_batch([pa.array([3 * i if i % 5 else None for i in range(40)], pa.int32()), pa.array(list(range(40)), pa.int64())], names=["r_k", "r_v"])}
    yield "semi_join", pc.join("Semi", left, right, [("l_k", "r_k")]).plan, build_query_dag, semi


CASES = {name: (plan, rule, rel) for name, plan, rule, rel in _cases()}


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_stages_over_the_model_give_the_whole_plans_rows(name, world):
    plan, rule, relations = CASES[name]
    tables = {k: _table(rb) for k, rb in relations.items()}
    whole = []
    for fields in pi.leaf_schemas(plan):
        want = [f["name"] for f in fields]
        t = next(t for t in tables.values() if set(t) <= set(want))
        n = len(next(iter(t.values())))
        whole.append({c: t.get(c, [None] * n) for c in want})
    names, _, want_rows = pi.run_plan(plan, whole)
    assert want_rows, "the case is vacuous"
    got_names, per_rank = model.run_stages(rule(plan), tables, world, pi.run_plan, pi.leaf_schemas)
    assert got_names == names
    assert multiset(rows_of_py([r for rows in per_rank for r in rows])) == multiset(rows_of_py(want_rows))
    if name == "golden_aggregate_sorted":      # the sort sits above a gather edge: rank 0 alone, in order
        assert rows_of_py(per_rank[0]) == rows_of_py(want_rows) and all(rows == [] for rows in per_rank[1:])


def test_the_model_keeps_source_rank_order_and_source_order():
    sent = [[(r, i) for i in range(5)] for r in range(3)]
    got = model.place(sent, lambda row: row[1] % 2, 3)
    assert got[0] == [(r, i) for r in range(3) for i in (0, 2, 4)] and got[1] == [(r, i) for r in range(3) for i in (1, 3)] and got[2] == []
    assert model.gather(sent, 2, 3) == [[], [], [row for rows in sent for row in rows]]
    assert [len(t["a"]) for t in model.stripe({"a": list(range(10))}, 3)] == [3, 3, 4]


def test_the_header_declares_the_entry_and_the_library_exports_it():
    from flock_amd import LIB_PATH
    header = open(os.path.join(ROOT, "include", "flockgpu_comm.h")).read()
    assert re.search(r"int\s+flockgpu_plan_exchange_retain\s*\(\s*flockgpu_plan\s*\*\s*plan,\s*flockgpu_comm\s*\*\s*comm,\s*int\s+gather_rank,\s*uint32_t\s+flags,\s*int64_t\s*\*\s*rows\s*\)\s*;", header)
    assert re.search(r"#define\s+FLOCKGPU_EXCHANGE_NO_ROWS\s+1u", header)
    lib = ctypes.CDLL(LIB_PATH)
    assert hasattr(lib, "flockgpu_plan_exchange_retain")


def test_the_python_surface_lists_the_entry_and_stagedrun_takes_a_communicator():
    from flock_amd import _ffi
    from flock_amd.runtime import ExecutionContext, _Plan
    from flock_amd.stages import StagedRun
    assert "flockgpu_plan_exchange_retain" in _ffi.SYMBOLS
    assert list(inspect.signature(_Plan.exchange_retain).parameters)[1:] == ["comm", "gather_rank", "no_rows"]
    assert list(inspect.signature(ExecutionContext.exchange_retain).parameters)[1:] == ["comm", "gather_rank", "no_rows"]
    assert "comm" in inspect.signature(StagedRun.__init__).parameters


def test_a_dag_that_needs_a_broadcast_edge_is_named():
    from flock_amd.stages import Stage, distributed_placement
    keyed = Stage(pc.hashed(pc.scan([("k", "Int32")]), "k"), [None])
    one_row = Stage(pc.aggregate(pc.scan([("m", "Int64")]), [], [("max", "m")], single="Partial").plan, [None])
    join = Stage({"execution_plan": "hash_join_exec"}, [0, 1])
    with pytest.raises(NotImplementedError, match="broadcast edge stage 1 -> stage 2"):
        distributed_placement([keyed, one_row, join])
    assert distributed_placement([keyed, Stage({"execution_plan": "memory_exec"}, [0])]) == (["key", "gather"], ["all", "all"])
