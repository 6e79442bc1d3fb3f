"""A plain-Python model of the distributed run of a stage DAG (`StagedRun(comm=...)` over flockgpu_plan_exchange_retain): stripe a table over
ranks, place rows by an arbitrary key function, concatenate what each rank receives in source-rank order.  With tests/plan_interp.run_plan
as the executor of a stage plan it gives the rows every rank's root stage must return -- without a GPU.

A table is {column: [values]}; rows are tuples in the table's column order; NULL is None."""
import zlib

from flock_amd.stages import distributed_placement, leaves_bfs


def stripe(table, world):
    """`world` tables: rank r takes the contiguous rows [n r / world, n (r + 1) / world)"""
    n = len(next(iter(table.values()))) if table else 0
    return [{k: v[n * r // world:n * (r + 1) // world] for k, v in table.items()} for r in range(world)]


def key_place(value, world):
    """A placement that is NOT the library's: which rank owns a key is unobservable in the union.  NULL is one key."""
    return zlib.crc32(repr(value).encode()) % world


def place(rows_per_rank, key_fn, world):
    """rows_per_rank[s]: the rows rank s sends, in its result order; key_fn(row) -> destination.  Returns what each rank receives: sources in
    rank order, a source's rows in their order."""
    got = [[] for _ in range(world)]
    for rows in rows_per_rank:
        for row in rows:
            got[key_fn(row)].append(row)
    return got


def gather(rows_per_rank, target, world):
    return place(rows_per_rank, lambda row: target, world)


def _root_hash_column(plan):
    while plan.get("execution_plan") == "coalesce_batches_exec":
        plan = plan["input"]
    return plan["partitioning"]["Hash"][0][0]["name"]


def run_stages(stages, relations, world, run_plan, leaf_schemas):
    """stages: flock_amd.stages.Stage list, leaves first; relations: {name: table} of the base relations (striped here); run_plan / leaf_schemas:
    tests/plan_interp's.  Returns (column names, per rank: the root stage's rows)."""
    edge, where = distributed_placement(stages)
    stripes = {name: stripe(t, world) for name, t in relations.items()}
    held = {}      # stage -> (names, per rank: rows received)
    for i, st in enumerate(stages):
        bfs = leaves_bfs(st.plan)
        produced, names = [[] for _ in range(world)], None
        for r in range(world):
            if where[i] == "zero" and r != 0:
                continue
            tables = []
            for fields in leaf_schemas(st.plan):
                want = [f["name"] for f in fields]
                at = next(k for k, lf in enumerate(bfs) if [f["name"] for f in lf["schema"]["fields"]] == want)
                src = st.inputs[at]
                if src is None:
                    rel = next(t[r] for t in stripes.values() if set(t[r]) <= set(want))
                    n = len(next(iter(rel.values())))
                    tables.append({c: rel.get(c, [None] * n) for c in want})
                else:
                    p_names, p_rows = held[src]
                    cols = list(zip(*p_rows[r])) if p_rows[r] else [[] for _ in p_names]
                    by_name = dict(zip(p_names, (list(c) for c in cols)))
                    tables.append({c: by_name[c] for c in want})
            names, _, rows = run_plan(st.plan, tables)
            produced[r] = rows
        if i == len(stages) - 1:
            return names, produced
        if edge[i] == "key":
            k = names.index(_root_hash_column(st.plan))
            held[i] = (names, place(produced, lambda row: key_place(row[k], world), world))
        else:
            held[i] = (names, gather(produced, 0, world))
