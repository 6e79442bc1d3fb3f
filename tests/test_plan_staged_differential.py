"""The random plans of tests/plan_corpus.py cut into stages -- by `build_query_dag` and by `split_at_repartitions` -- and run stage by stage: over the
ranks of a communicator (`StagedRun(gpu, stages, comm=...)`, every rank over its contiguous stripe of every table) and on one device
(`instances=1`, with and without `on_device`), against the row-at-a-time interpreter of tests/plan_interp.py, by the rules of
tests/test_plan_differential.py: names and Arrow types, Float64 by its bits, Timestamp as Int64, Utf8 as bytes; rows in sequence where the case is
ordered (and then on rank 0 alone, the root stage running there), as a multiset otherwise.

The CPU part holds `distributed_placement` to the model of tests/plan_exchange_model.py with the interpreter as the executor of every stage: a
stage DAG it ACCEPTS gives the whole plan's rows at worlds 2 and 3, a DAG it REFUSES is refused by stage and node kind.  Acceptance is asserted
(`test_the_accepted_set_has_its_floors`), never used to filter what is compared.

Two sets of cases are out of scope, each pinned to exactly the cases it names (`test_the_exclusions_are_exactly_the_named_sets`):
  * plans with a `distinct_count` entry: the cut between Partial and Final of a distinct count is refused by the library
    (tests/test_plan_count_distinct.py);
  * plans whose root is a lone Partial aggregate: one partial row per rank is a correct answer, but not the whole plan's."""
import functools
import json
import re

import pytest

import plan_corpus as pc
import plan_exchange_model as model
import plan_interp as pi
from flock_amd.stages import Stage, build_query_dag, distributed_placement, split_at_repartitions
from test_gpu_plan_exchange import multiset, rows_of, run_ranks
from test_plan_differential import SEEDS, _arrow, _batches, _case, _multiset, _norm, _want

RULES = (("build_query_dag", build_query_dag), ("split_at_repartitions", split_at_repartitions))
STRATA = [s for s in pc.STRATA if s not in pc.ERROR_STRATA and s != "distinct_count"]      # (every case of distinct_count is excluded, see below)
WORLDS = (2, 3)
MODEL_ROWS = 9000          # the CPU model runs the cases of up to this many rows: 22 of the 24 of a stratum (the two larger ones are the same recipes)


# ------------------------------------------------------------------ the cases in scope
def _nodes(plan):
    out = [plan]
    for k in ("input", "left", "right"):
        if isinstance(plan.get(k), dict):
            out += _nodes(plan[k])
    for x in plan.get("inputs") or ():
        out += _nodes(x)
    return out


def _kinds(plan):
    return {n.get("execution_plan") for n in _nodes(plan)}


def _excluded(plan):
    """the name of the exclusion the plan falls under, or None"""
    if any(e.get("aggregate_expr") == "distinct_count" for n in _nodes(plan) for e in n.get("aggr_expr") or ()):
        return "distinct_count"
    if plan.get("execution_plan") == "hash_aggregate_exec" and plan.get("mode") == "Partial":
        return "lone_partial"
    return None


@functools.lru_cache(maxsize=None)
def _keys(stratum):
    """-> (the (stratum, seed, i) in scope, {exclusion: [keys]})"""
    scope, out = [], {}
    for seed in SEEDS:
        for i in range(pc.CASES_PER_SEED):
            why = _excluded(_case(stratum, seed, i).plan)
            if why:
                out.setdefault(why, []).append((stratum, seed, i))
            else:
                scope.append((stratum, seed, i))
    return scope, out


def _rows_in(key):
    return max(len(next(iter(t.values()))) for t in _case(*key).tables)


def test_the_exclusions_are_exactly_the_named_sets():
    got = {}
    for s in pc.STRATA:
        if s not in pc.ERROR_STRATA:
            for why, keys in _keys(s)[1].items():
                got.setdefault(why, set()).update(keys)
    assert _keys("distinct_count")[0] == [] and all(_keys(s)[0] for s in STRATA)
    every = [(seed, i) for seed in SEEDS for i in range(pc.CASES_PER_SEED)]
    assert got.pop("distinct_count") == {("distinct_count", seed, i) for seed, i in every} | {("cast_text", seed, 3) for seed in SEEDS}
    assert got.pop("lone_partial") == {("global_agg", seed, 5) for seed in SEEDS}
    assert not got


# ------------------------------------------------------------------ the stage DAGs of a case
class Dag:
    """the stages one or both splitters give for a case, and what distributed_placement says to them"""
    def __init__(self, rules, stages):
        self.rules, self.stages = rules, stages
        try:
            self.edge, self.where = distributed_placement(stages)
            self.refusal = None
        except NotImplementedError as e:
            self.edge = self.where = None
            self.refusal = str(e)

    @property
    def accepted(self):
        return self.refusal is None

    @property
    def on_zero(self):
        return self.where[-1] == "zero"


@functools.lru_cache(maxsize=None)
def _dags(key):
    """one Dag per distinct list of stage plans: a plan both splitters cut alike is run once"""
    out, seen = [], {}
    for name, rule in RULES:
        stages = rule(_case(*key).plan)
        text = json.dumps([[st.plan, st.inputs] for st in stages], sort_keys=True)
        if text in seen:
            seen[text].rules += (name,)
        else:
            seen[text] = Dag((name,), stages)
            out.append(seen[text])
    return out


def _dag_of(key, rule):
    return next(d for d in _dags(key) if rule in d.rules)


@functools.lru_cache(maxsize=None)
def _want_rows(key):
    """the interpreter's rows of the case, normalised: (in sequence, as a multiset) -- computed once, shared and left unchanged"""
    rows = _norm(_want(*key)[2])
    return rows, _multiset(rows)


def _compare_rows(per_rank, key, dag, ordered, where):
    """per_rank: the root stage's rows of every rank, normalised.  A root stage on rank 0 leaves the other ranks empty, and its rows are compared in
    sequence where the case defines one (`ordered`: an accepted DAG has such a sort on rank 0).  Everything else is a multiset -- an ordered union
    that runs on every rank, and an unordered root on rank 0: mixed case 1, a window over a sort over a join, sorts rows that tie on its keys as
    they arrive, and a gathered join hands them over in another order than the whole plan's join does."""
    got = [row for rows in per_rank for row in rows]
    if dag.on_zero:
        assert all(rows == [] for rows in per_rank[1:]), where
    a, b = (got, _want_rows(key)[0]) if ordered and dag.on_zero else (_multiset(got), _want_rows(key)[1])
    if a != b:
        diff = [(k, x, y) for k, (x, y) in enumerate(zip(a, b)) if x != y][:3]
        pytest.fail("%d rows, %d expected; first differing (position, got, expected): %r\n%s" % (len(a), len(b), diff or (a[len(b):][:3], b[len(a):][:3]), where))


def _check_refusal(dag, where):
    """the message names a stage and a node kind of that stage's plan -- or, the broadcast refusal, an edge of the DAG"""
    m = re.search(r"broadcast edge stage (\d+) -> stage (\d+)", dag.refusal)
    if m:
        g, i = int(m.group(1)), int(m.group(2))
        assert i < len(dag.stages) and g in dag.stages[i].inputs, (where, dag.refusal)
        return
    m = re.search(r"stage (\d+) .* its (\w+_exec)", dag.refusal)
    assert m, (where, dag.refusal)
    assert int(m.group(1)) < len(dag.stages) and m.group(2) in _kinds(dag.stages[int(m.group(1))].plan), (where, dag.refusal)


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("stratum", STRATA)
def test_placement_accepts_only_what_the_model_confirms(stratum):
    """every DAG distributed_placement accepts gives, over the model, the interpreter's names and rows; every DAG it refuses is refused by name"""
    ran = 0
    for key in _keys(stratum)[0]:
        if _rows_in(key) > MODEL_ROWS:
            continue
        c = _case(*key)
        names = _want(*key)[0]
        relations = {"r%d" % k: t for k, t in enumerate(c.tables)}
        for dag in _dags(key):
            where = "case%r %s (%s)" % (key, "/".join(dag.rules), c.note)
            if not dag.accepted:
                _check_refusal(dag, where)
                continue
            for world in WORLDS:
                got_names, per_rank = model.run_stages(dag.stages, relations, world, pi.run_plan, pi.leaf_schemas)
                assert got_names == names, where
                _compare_rows([_norm(r) for r in per_rank], key, dag, c.ordered, "%s world %d" % (where, world))
                ran += 1
    assert ran or stratum == "cross", stratum


ALL_BY_BUILD_QUERY_DAG = ("filter_project", "text", "group_narrow", "group_composite", "group_wide", "join_inner", "join_semi_anti", "sort_limit", "window",
                          "parse_text", "global_agg", "cast_text")          # (the last two: every case in scope)
ALL_BY_SPLIT = ("filter_project", "text", "group_composite", "group_wide", "join_semi_anti")


def _accepted(stratum, rule):
    return [key for key in _keys(stratum)[0] if _dag_of(key, rule).accepted]


def test_the_accepted_set_has_its_floors():
    """conditions, not measurements: where the cut is sound the DAG must be accepted, every size included"""
    for s in ALL_BY_BUILD_QUERY_DAG:
        assert _accepted(s, "build_query_dag") == _keys(s)[0], (s, [(k, _dag_of(k, "build_query_dag").refusal) for k in _keys(s)[0] if not _dag_of(k, "build_query_dag").accepted][:2])
    for s in ALL_BY_SPLIT:
        assert _accepted(s, "split_at_repartitions") == _keys(s)[0], (s, [(k, _dag_of(k, "split_at_repartitions").refusal) for k in _keys(s)[0] if not _dag_of(k, "split_at_repartitions").accepted][:2])
    for name, _ in RULES:
        assert _accepted("cross", name) == []
    assert not [k for k in _accepted("mixed", "build_query_dag") if k[2] == 3]
    for s in ("filter_project", "text", "group_narrow", "join_inner", "sort_limit", "window", "global_agg"):
        assert len(_keys(s)[0]) == len(SEEDS) * pc.CASES_PER_SEED - sum(len(v) for v in _keys(s)[1].values())


# ------------------------------------------------------------------ refusals written out by hand: literal plans, no generator
def _label_counts():
    a = pc.scan([("label", "Utf8"), ("v", "Int64")])
    return pc.aggregate(a, ["label"], [("count", None), ("sum", "v")])


def _refusal_of(stages):
    with pytest.raises(NotImplementedError) as e:
        distributed_placement(stages)
    return str(e.value)


def test_a_semi_join_over_an_aggregate_with_its_repartition_in_one_stage_is_refused_by_name():
    """the shape of mixed (seeds 0 and 2, case 2): Semi(Repartition(FinalPartitioned(Repartition(Partial(scan)))), Repartition(scan)).  build_query_dag
    stops at the join, so its left input is ONE stage with a hash repartition in its middle: over stripes every rank would finish the aggregate on
    its own stripe -- a label that stands in two stripes would come out twice, with two partial counts."""
    plan = pc.join("Semi", _label_counts(), pc.scan([("b_s", "Utf8")]), [("label", "b_s")]).plan
    stages = build_query_dag(plan)
    left = next(k for k, st in enumerate(stages) if "hash_aggregate_exec" in _kinds(st.plan))
    assert [n.get("execution_plan") for n in _nodes(stages[left].plan)].count("repartition_exec") == 2
    msg = _refusal_of(stages)
    assert "stage %d " % left in msg and "hash_aggregate_exec" in msg and "split_at_repartitions" in msg, msg
    # cut at every repartition the same plan is sound: accepted, and the model gives the whole plan's rows where a label spans the stripes
    tables = [{"label": ["a", "b", "a", None, "b", "c", "a", "c"], "v": [1, 2, 3, 4, 5, 6, 7, None]}, {"b_s": ["a", "c", "zz", None]}]
    names, _, rows = pi.run_plan(plan, tables)
    assert sorted(rows) == [("a", 3, 11), ("c", 2, 6)]
    finer = split_at_repartitions(plan)
    assert distributed_placement(finer)[1] == ["all"] * len(finer)
    for world in WORLDS:
        got_names, per_rank = model.run_stages(finer, {"a": tables[0], "b": tables[1]}, world, pi.run_plan, pi.leaf_schemas)
        assert got_names == names and sorted(r for rows_r in per_rank for r in rows_r) == sorted(rows)


def test_a_sort_over_a_striped_input_is_refused_by_name():
    """a sort that runs on every rank sorts a stripe (or a partition): the ranks' results are no sorted whole.  split_at_repartitions leaves a sort
    over an aggregate in the stage of the FinalPartitioned, which runs on every rank; build_query_dag cuts below the sort, a gather edge."""
    a = pc.scan([("k", "Int32"), ("v", "Int64")])
    msg = _refusal_of([Stage(pc.sort(a, [("k", False, False)]).plan, [None])])
    assert "stage 0 " in msg and "sort_exec" in msg and "gather edge" in msg, msg
    plan = pc.sort(pc.aggregate(a, ["k"], [("sum", "v")]), [("k", False, False)]).plan
    finer = split_at_repartitions(plan)
    assert [st.plan["execution_plan"] for st in finer] == ["coalesce_batches_exec", "sort_exec"]
    msg = _refusal_of(finer)
    assert "stage 1 " in msg and "sort_exec" in msg, msg
    assert distributed_placement(build_query_dag(plan)) == (["key", "gather", "gather"], ["all", "all", "zero"])
    for node in (pc.limit(a, 3), pc.window(a, [("row_number", None, ["k"], [])])):
        msg = _refusal_of([Stage(node.plan, [None])])
        assert "stage 0 " in msg and node.plan["execution_plan"] in msg, msg
    # a Final aggregate over a stripe, and a gather below the root of a stage on every rank
    final = pc.aggregate(a, [], [("max", "v")]).plan
    assert final["mode"] == "Final" and final["input"]["execution_plan"] == "coalesce_partitions_exec"
    msg = _refusal_of([Stage(final, [None])])
    assert "stage 0 " in msg and "hash_aggregate_exec (Final)" in msg, msg
    msg = _refusal_of([Stage(pc.filt(pc.Node(final["input"], []), pc.lit("Int32", 1)).plan, [None])])
    assert "stage 0 " in msg and "coalesce_partitions_exec" in msg, msg
    assert distributed_placement(build_query_dag(final)) == (["gather", "gather"], ["all", "zero"])          # the gather AT the root is the edge itself


def test_a_cross_join_of_two_striped_scans_is_refused_by_name():
    """stripe r of the left crossed with stripe r of the right: world * (n / world)^2 pairs out of n^2"""
    plan = pc.cross(pc.scan([("a", "Int32")]), pc.scan([("b", "Int32")])).plan
    for stages in (build_query_dag(plan), split_at_repartitions(plan), [Stage(plan, [None, None])]):
        msg = _refusal_of(stages)
        assert "stage 0 " in msg and "cross_join_exec" in msg, msg


def test_a_partitioned_join_or_aggregate_needs_key_edges_and_a_stage_on_rank_zero_takes_anything():
    a, b = pc.scan([("x", "Int32"), ("s", "Utf8")]), pc.scan([("y", "Int32")])
    j = pc.join("Inner", a, b, [("x", "y")])
    bare = dict(j.plan, left=a.plan, right=b.plan)          # the join over its two leaves
    keyed = [Stage(pc.hashed(a, "x"), [None]), Stage(pc.hashed(b, "y"), [None])]
    assert distributed_placement(keyed + [Stage(bare, [0, 1])]) == (["key", "key", "gather"], ["all", "all", "all"])
    assert distributed_placement(keyed + [Stage(dict(bare, left=pc.filt(a, pc.binop(a.c("x"), "Gt", pc.lit("Int32", 0))).plan), [0, 1])])[1][2] == "all"
    for inputs in ([None, None], [0, None]):                 # a base relation below a Partitioned join: striped, not partitioned by the key
        msg = _refusal_of(keyed + [Stage(bare, inputs)])
        assert "stage 2 " in msg and "hash_join_exec" in msg, msg
    msg = _refusal_of([Stage(j.plan, [None, None])])          # the join with both of its repartitions in one stage
    assert "stage 0 " in msg and "hash_join_exec" in msg and "split_at_repartitions" in msg, msg
    # everything gathered: the stage runs on rank 0 and takes a sort, a limit and a cross join alike
    gathered = [Stage(a.plan, [None]), Stage(b.plan, [None])]
    top = pc.limit(pc.sort(pc.cross(a, b), [("x", False, False)]), 5)
    assert distributed_placement(gathered + [Stage(top.plan, [0, 1])]) == (["gather"] * 3, ["all", "all", "zero"])


# ------------------------------------------------------------------ GPU
def _relations(c, poison=None):
    """one whole RecordBatch per relation of the case, built the way the differential builds its batches (poison: what lies under the NULLs)"""
    return {"r%d" % k: bs[0] for k, bs in enumerate(_batches(c.plan, c.tables, [None] * len(c.tables), poison=poison))}


def _stripe(rb, r, world):
    lo, hi = rb.num_rows * r // world, rb.num_rows * (r + 1) // world
    return rb.slice(lo, hi - lo)


def _same_batches(a, b):
    return len(a) == len(b) and all(x.equals(y) for x, y in zip(a, b))


def _check_schema(batches, key, where):
    names, types, _ = _want(*key)
    for rb in batches:
        if rb.num_rows:
            assert rb.schema.names == names, where
            assert [f.type for f in rb.schema] == [_arrow(t) for t in types], where


def _jobs(stratum, seed, accepted_only):
    return [(key, dag) for key in _keys(stratum)[0] if key[1] == seed for dag in _dags(key) if dag.accepted or not accepted_only]


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("stratum", STRATA)
def test_gpu_staged_ranks_equal_the_interpreter(stratum, seed, world):
    """every accepted DAG of every case in scope through StagedRun(comm=...) on `world` thread ranks of device 0, twice through the same instances"""
    from flock_amd.stages import StagedRun
    jobs = _jobs(stratum, seed, True)
    relations = {key: _relations(_case(*key)) for key, _ in jobs}

    def body(r, gpu, comm):
        out, ran = [], set()
        for key, dag in jobs:
            run = StagedRun(gpu, dag.stages, comm=comm)
            if r == 0:                                           # (per DAG: profile_read gives 64 names at the most)
                gpu.profile_reset()
                gpu.profile(True)
            try:
                mine = {k: _stripe(rb, r, world) for k, rb in relations[key].items()}
                first = run.run(mine)
                again = run.run(mine)                            # the plans are reusable: a second window through the same instances
                if r == 0:
                    ran |= set(gpu.profile_read())
            finally:
                if r == 0:
                    gpu.profile(False)
                run.close()
            out.append((first, None if _same_batches(first, again) else again))
        return out, ran

    results = run_ranks(world, body) if jobs else []
    for at, (key, dag) in enumerate(jobs):
        c = _case(*key)
        where = "case%r %s world %d (%s)" % (key, "/".join(dag.rules), world, c.note)
        per_rank = []
        for r in range(world):
            first, again = results[r][0][at]
            _check_schema(first, key, where)
            rows = _norm(rows_of(first))
            if again is not None:
                assert multiset(_norm(rows_of(again))) == multiset(rows), "the second run differs from the first: " + where
            per_rank.append(rows)
        _compare_rows(per_rank, key, dag, c.ordered, where)
    if any("key" in dag.edge[:-1] for _, dag in jobs):           # against a vacuous pass: some result went through the partition's emit pass
        ran = results[0][1]
        assert any(name.startswith("partition_emit_table_kernel") for name in ran), (stratum, seed, world, sorted(ran))
    elif stratum not in ("cross",):
        assert jobs, (stratum, seed)


@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("stratum", STRATA)
def test_gpu_staged_on_one_device_equals_the_interpreter(gpu, stratum, seed):
    """every DAG of every case in scope, accepted for a distributed run or not: one instance per stage over whole relations is sound for every DAG.
    Seed 0 runs once more with tests/null_poison.py's far pool under every NULL of the relations: the hand-over between stages -- the exchange's
    packing, the hash partitioning -- sees hostile slots too, and validity alone decides"""
    from flock_amd.stages import StagedRun
    for key, dag in _jobs(stratum, seed, False):
        c = _case(*key)
        want = _want_rows(key)[0 if c.ordered else 1]
        for poison in (None, ("far", key)) if seed == 0 else (None,):
            relations = _relations(c, poison)
            for on_device in (False, True):
                where = "case%r %s on_device=%s poison=%s (%s)" % (key, "/".join(dag.rules), on_device, poison and poison[0], c.note)
                run = StagedRun(gpu, dag.stages, instances=1, on_device=on_device)
                try:
                    out = run.run(relations)
                finally:
                    run.close()
                _check_schema(out, key, where)
                got = _norm(rows_of(out))
                if not c.ordered:
                    got = _multiset(got)
                if got != want:
                    diff = [(k, a, b) for k, (a, b) in enumerate(zip(got, want)) if a != b][:3]
                    pytest.fail("%d rows, %d expected; first differing (position, got, expected): %r\n%s" % (len(got), len(want), diff or (got[len(want):][:3], want[len(got):][:3]), where))


# ------------------------------------------------------------------ a row that fails the execute, on one rank of three
PER_RANK = 1000
BAD = (1, 617)      # (rank, row of its stripe)


def _failing(kind):
    """-> (cols of the producer's leaf, producer plan, cols of its result, per rank: the table with the ONE bad row in rank 1's stripe, the value that repairs it)"""
    n = 3 * PER_RANK
    k = [(j * 7919) % 97 - 40 for j in range(n)]
    if kind == "zero_divisor":                                   # i / j in a projection under the root repartition
        cols = [("k", "Int64"), ("i", "Int32"), ("j", "Int32")]
        a = pc.scan(cols)
        below = pc.proj(a, [(a.c("k"), "k", "Int64"), (pc.binop(a.c("i"), "Divide", a.c("j")), "q", "Int32")])
        table = {"k": k, "i": [j * 3 - 1000 for j in range(n)], "j": [j % 5 + 1 for j in range(n)]}
        name, bad, good = "j", 0, 2
    elif kind == "text_in_a_filter":                             # CAST(s AS Int64) in a predicate directly below the repartition: the composed filter_rows path
        cols = [("k", "Int64"), ("s", "Utf8")]
        a = pc.scan(cols)
        below = pc.filt(a, pc.binop(pc.cast(a.c("s"), "Int64"), "Gt", pc.lit("Int64", 500)))
        table = {"k": k, "s": [str(j % 1000) for j in range(n)]}
        name, bad, good = "s", "12x", "712"
    else:                                                        # CAST(t AS Utf8) of a timestamp beyond the year 9999
        assert kind == "year_10000"
        cols = [("k", "Int64"), ("t", "ts")]
        a = pc.scan(cols)
        below = pc.proj(a, [(a.c("k"), "k", "Int64"), (pc.cast(a.c("t"), "Utf8"), "w", "Utf8")])
        table = {"k": k, "t": [1_436_918_400_000 + 86_399_123 * j for j in range(n)]}
        name, bad, good = "t", pc.TS_MAX + 1, pc.TS_MAX
    at = BAD[0] * PER_RANK + BAD[1]
    broken, repaired = dict(table), dict(table)
    broken[name] = table[name][:at] + [bad] + table[name][at + 1:]
    repaired[name] = table[name][:at] + [good] + table[name][at + 1:]
    return cols, pc.hashed(below, "k"), below.cols, broken, repaired


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zero_divisor", "text_in_a_filter", "year_10000"])
def test_a_row_that_fails_on_one_rank_fails_every_rank(kind):
    """the rank whose stripe holds the bad row raises what the whole plan's execute raises over that stripe (FLOCKGPU_ERR_INVALID, the same
    message), the other two FLOCKGPU_ERR_PEER naming it -- nobody is left waiting --, and the same plans then exchange the repaired table"""
    from flock_amd import FlockGpuError, _ffi
    from flock_amd.runtime import collect
    from test_gpu_plan_exchange import Pair, batch
    world = 3
    cols, producer, out_cols, broken, repaired = _failing(kind)
    stripes = [[{c: v[PER_RANK * r:PER_RANK * (r + 1)] for c, v in t.items()} for r in range(world)] for t in (broken, repaired)]

    def body(r, gpu, comm):
        pair = Pair(gpu, producer, pc.scan(out_cols).plan)
        whole = None
        try:
            if r == BAD[0]:      # the whole plan's execute over this stripe, on the same plan instance (its messages name the instance)
                try:
                    collect(pair.p, [[[batch(stripes[0][r], cols)]]])
                except FlockGpuError as e:
                    whole = (e.code, str(e))
                finally:
                    pair.p.clean_data_sources()
            try:
                pair.exchange(comm, stripes[0][r], cols)
                err = None
            except FlockGpuError as e:
                err = (e.code, str(e))
            return err, pair.exchange(comm, stripes[1][r], cols), whole
        finally:
            pair.close()
    out = run_ranks(world, body)
    whole = out[BAD[0]][2]
    print("\n%s: whole plan %r\nranks %r" % (kind, whole, [o[0] for o in out]))
    assert whole is not None and whole[0] == _ffi.ERR_INVALID, whole
    assert out[BAD[0]][0] == whole
    for r in (0, 2):
        assert out[r][0] is not None and out[r][0][0] == _ffi.ERR_PEER and "rank %d" % BAD[0] in out[r][0][1], (r, out[r][0])
    want = pi.run_plan(producer, [repaired])[2]
    assert want and multiset(_norm([row for o in out for row in o[1]])) == multiset(_norm(want))
    assert sum(1 for o in out if o[1]) > 1


# ------------------------------------------------------------------ findings, reduced: literal plans and tables, no generator
def _scan_beside_an_aggregate():
    b, a = pc.scan([("x", "Int32"), ("n", "UInt64")]), pc.scan([("k", "Int32"), ("v", "Int64")])
    plan = pc.union([b, pc.aggregate(a, ["k"], [("count", None)])]).plan
    tables = [{"x": [1, 2, None], "n": [10, 20, 30]}, {"k": [None if j % 11 == 0 else j % 7 for j in range(50)], "v": list(range(50))}]
    return plan, tables, [[None], [None, 0]], 3 + 8


def _scan_beside_a_join():
    a = pc.scan([("p", "Int32"), ("q", "Int32")])
    c, b = pc.scan([("c_k", "Int32"), ("c_v", "Int32"), ("c_w", "Int64")]), pc.scan([("b_k", "Int32"), ("b_v", "Int32")])
    j = pc.join("Inner", pc.keep(c, ["c_k", "c_v"]), pc.keep(b, ["b_k", "b_v"]), [("c_k", "b_k")])
    plan = pc.union([a, pc.keep(j, ["c_v", "b_v"])]).plan
    tables = [{"p": [5, None], "q": [6, 7]}, {"c_k": [j % 50 for j in range(200)], "c_v": list(range(200)), "c_w": [None] * 200},
              {"b_k": [(j * 7) % 50 for j in range(100)], "b_v": list(range(100))}]
    return plan, tables, [[None], [None], [None, 0, 1]], 2 + 400


@pytest.mark.gpu
@pytest.mark.parametrize("make", [_scan_beside_an_aggregate, _scan_beside_a_join])
def test_a_stage_reads_a_base_relation_next_to_its_producers(gpu, make):
    """Found by union (case 5 of every seed, split_at_repartitions): UNION ALL of a scan and an aggregate -- or a join --, cut at the repartitions,
    is a stage with one leaf on a base relation and the others on the stages below.  StagedRun fed such a stage its base relations alone on one
    device: the other leaves stayed empty relations and their rows were missing from the result, without an error.  Over a communicator feed_from
    stopped at the leaf that held the relation (`plan_feed_from: input 0 already holds rows`).  And a join input cut off above the projection
    of a relation (seed 2) still carries that relation's column names: fed every relation, its leaf took the rank's STRIPE of the relation in
    place of the partition the stage below had sent, and the join lost the pairs that span two stripes."""
    from flock_amd.stages import StagedRun
    plan, tables, inputs, n_rows = make()
    stages = split_at_repartitions(plan)
    assert [st.inputs for st in stages] == inputs and distributed_placement(stages)[1] == ["all"] * len(stages)
    rows = pi.run_plan(plan, tables)[2]
    assert len(rows) == n_rows
    want = _multiset(_norm(rows))
    relations = {"r%d" % k: bs[0] for k, bs in enumerate(_batches(plan, tables, [None] * len(tables)))}
    for on_device in (False, True):
        run = StagedRun(gpu, stages, instances=1, on_device=on_device)
        try:
            assert _multiset(_norm(rows_of(run.run(relations)))) == want, on_device
        finally:
            run.close()
    for world in WORLDS:
        def body(r, ctx, comm):
            run = StagedRun(ctx, stages, comm=comm)
            try:
                return rows_of(run.run({k: _stripe(rb, r, world) for k, rb in relations.items()}))
            finally:
                run.close()
        assert _multiset(_norm([row for got in run_ranks(world, body) for row in got])) == want, world
