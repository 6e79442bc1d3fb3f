"""flockgpu_plan_exchange_retain (include/flockgpu_comm.h): the result of a stage plan hash-partitioned over the ranks of a communicator -- or
gathered on one -- by the library's own all-to-all, and left on the device for flockgpu_plan_feed_from.

Ranks are threads of this process on device 0 over the `local` transport (as tests/test_gpu_comm.py runs the query exchanges).  The producer is
`memory_exec` under `repartition_exec Hash([k], 4)`, the consumer a bare `memory_exec` of the same schema executed to the host, so what a rank's
consumer returns IS what the exchange left on that rank.  Comparisons are exact: multisets of row tuples (floats by their bits), and the
order inside a rank through the hidden column `src` = (rank << 32) | row."""
import struct
import threading

import numpy as np
import pyarrow as pa
import pytest

import plan_corpus as pc

pytestmark = pytest.mark.gpu

TILE = 8192   # partition tile and flag tile alike
COLS = [("k32", "Int32"), ("k64", "Int64"), ("ku", "UInt64"), ("kt", "ts"), ("f", "Float64"), ("s0", "Utf8"), ("s1", "Utf8"), ("s2", "Utf8"),
        ("s3", "Utf8"), ("s4", "Utf8"), ("src", "Int64")]
KEYS = ["k32", "k64", "ku", "kt", "s0"]
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string(), "ts": pa.timestamp("ms")}
TEXTS = ["", "a", "x" * 17, "y" * 70, "été €", "z" * 5000]


def make_table(rank, n, seed, nulls=0.2, constant_key=False):
    """n rows of COLS for one rank: every key column over ~40 distinct values that every rank draws from; NULLs in every column but `src`."""
    r = np.random.default_rng(1000 * seed + rank)
    d = r.integers(0, 40, n)
    if constant_key:
        d = np.full(n, 7)
    t = {"k32": [int(x) * 100003 - 17 for x in d],
         "k64": [int(x) * (2**40 + 3) - 2**50 for x in d],
         "ku": [2**63 - 20 + int(x) for x in d],
         "kt": [int(x) * 86_400_123 - 10**11 for x in d],
         "f": [int(x) / 4 for x in r.integers(-2**20, 2**20, n)],
         "s0": [TEXTS[int(x) % 5] + ("" if x < 5 else "k%d" % x) for x in d],
         "s1": [TEXTS[int(x)] for x in r.integers(0, 5, n)],
         "s2": [TEXTS[5] if x == 0 else "v%d" % x for x in r.integers(0, 600, n)],      # a 5000-byte value now and then
         "s3": ["" for _ in range(n)],
         "s4": [TEXTS[int(x)] * 2 for x in r.integers(0, 5, n)]}
    out = {}
    for name, _ in COLS[:-1]:
        share = 0.0 if constant_key and name in KEYS else nulls
        out[name] = pc.with_nulls(t[name], share, r)
    out["src"] = [(rank << 32) | i for i in range(n)]
    return out


def batch(table, cols=COLS):
    arrs = []
    for name, ty in cols:
        arrs.append(pa.array(table[name], pa.int64()).cast(_PA[ty]) if ty == "ts" else pa.array(table[name], _PA[ty]))
    return pa.record_batch(arrs, names=[n for n, _ in cols])


def rows_of(batches):
    rows = []
    for rb in batches:
        cols = [(c.cast(pa.int64()) if pa.types.is_timestamp(c.type) else c).to_pylist() for c in rb.columns]
        rows += list(zip(*cols)) if cols else []
    return [tuple(("f", struct.unpack("<q", struct.pack("<d", v))[0]) if isinstance(v, float) else v for v in r) for r in rows]


def table_rows(table, cols=COLS):
    return rows_of([batch(table, cols)])


def multiset(rows):
    return sorted(rows, key=lambda r: tuple((0, 0) if v is None else (1, repr(type(v)), v) for v in r))


def producer_plan(key, cols=COLS, below=None):
    node = below or pc.scan(cols)
    return pc.hashed(node, key)


def run_ranks(world, body, piece=None):
    """body(rank, gpu, comm) on `world` threads, each with a GpuContext of its own (own stream) on device 0; returns the results."""
    import torch
    from flock_amd import Comm, GpuContext
    comms = Comm.local(world)
    if piece:
        for c in comms:
            c.set_max_piece_bytes(piece)
    ctxs = [GpuContext(0, own_stream=True) for _ in range(world)]
    out, err = [None] * world, [None] * world
    torch.cuda.synchronize()

    def run(r):
        try:
            out[r] = body(r, ctxs[r], comms[r])
        except BaseException as e:      # noqa: BLE001 -- surfaced below; a dead rank would leave the others at a barrier
            err[r] = e
    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    alive = [t.is_alive() for t in threads]
    assert not any(alive), "a rank is stuck in the exchange"
    for e in err:
        if e is not None:
            raise e
    for c in comms:
        c.close()
    for c in ctxs:
        c.close()
    return out


class Pair:
    """One rank's producer and consumer plan."""

    def __init__(self, gpu, producer, consumer):
        from flock_amd.runtime import ExecutionContext
        self.p = ExecutionContext([producer], gpu=gpu, generic_only=True)
        self.c = ExecutionContext([consumer], gpu=gpu, generic_only=True)

    def exchange(self, comm, table, cols=COLS, gather_rank=-1, no_rows=False):
        """feed -> exchange_retain -> feed_from -> execute -> clean: (rows the entry reported, the consumer's rows)"""
        try:
            if table is not None and len(table[cols[0][0]]):
                self.p.feed_data_sources([[[batch(table, cols)]]])
            n = self.p.exchange_retain(comm, gather_rank, no_rows)[0]
            self.c.feed_from([self.p])
            got = rows_of(self.c.execute()[0])
        finally:
            self.c.clean_data_sources()
            self.p.clean_data_sources()
        assert n == len(got)
        return got

    def close(self):
        self.c.close()
        self.p.close()


def exchange_once(world, tables, key="k64", cols=COLS, gather_rank=-1, no_rows=(), piece=None, plan=None, consumer=None):
    plan = plan or producer_plan(key, cols)
    consumer = consumer or pc.scan(cols).plan

    def body(r, gpu, comm):
        pair = Pair(gpu, plan, consumer)
        try:
            return pair.exchange(comm, tables[r], cols, gather_rank, r in no_rows)
        finally:
            pair.close()
    return run_ranks(world, body, piece)


def check_order(got_per_rank, src_col=len(COLS) - 1):
    """every rank's rows: sources in rank order, inside a source in source order"""
    for got in got_per_rank:
        tags = [r[src_col] for r in got]
        assert tags == sorted(tags), "rows are not a concatenation of per-source subsequences in rank order"


def check_placement(got_per_rank, key_col):
    seen = [set(r[key_col] for r in got) for got in got_per_rank]
    for a in range(len(seen)):
        for b in range(a + 1, len(seen)):
            assert not (seen[a] & seen[b]), "ranks %d and %d both hold key(s) %r" % (a, b, sorted(seen[a] & seen[b], key=repr)[:3])
    assert sum(1 for s in seen if None in s) <= 1, "NULL-keyed rows sit on more than one rank"


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("key", KEYS)
def test_every_key_type_places_equal_keys_on_one_rank(key, world):
    tables = [make_table(r, 3000 + 11 * r, seed=KEYS.index(key)) for r in range(world)]
    got = exchange_once(world, tables, key)
    want = [row for t in tables for row in table_rows(t)]
    assert multiset([row for g in got for row in g]) == multiset(want)
    check_placement(got, [n for n, _ in COLS].index(key))
    check_order(got)
    assert sum(1 for g in got if g) > 1, "every row went to one rank"


def test_four_ranks():
    tables = [make_table(r, 2500, seed=9) for r in range(4)]
    got = exchange_once(4, tables, "k32")
    assert multiset([row for g in got for row in g]) == multiset([row for t in tables for row in table_rows(t)])
    check_placement(got, 0)
    check_order(got)


def test_six_ranks_take_the_one_pass_emit():
    """above four destinations the emit pass builds every destination's list in one pass (another kernel than the loop of the cases above)"""
    tables = [make_table(r, TILE + 300 if r == 2 else 1500, seed=17) for r in range(6)]
    got = exchange_once(6, tables, "ku")
    assert multiset([row for g in got for row in g]) == multiset([row for t in tables for row in table_rows(t)])
    check_placement(got, 2)
    check_order(got)


@pytest.mark.parametrize("shape", ["none", "one_rank_only", "one_row", TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_rows_per_rank_around_the_tile_boundaries(shape):
    world = 3
    counts = {"none": [0, 0, 0], "one_rank_only": [0, 700, 0], "one_row": [1, 1, 1]}.get(shape) or [shape] * world
    tables = [make_table(r, n, seed=3) for r, n in enumerate(counts)]
    got = exchange_once(world, tables, "k64")
    assert multiset([row for g in got for row in g]) == multiset([row for t in tables for row in table_rows(t)])
    check_placement(got, 1)
    check_order(got)


def test_one_key_goes_to_one_rank_and_the_others_receive_nothing():
    world = 3
    tables = [make_table(r, 5000, seed=4, constant_key=True) for r in range(world)]
    got = exchange_once(world, tables, "k64")
    assert sorted(len(g) for g in got) == [0, 0, 15000]
    full = next(g for g in got if g)
    assert full == [row for t in tables for row in table_rows(t)]       # rank order, source order: the concatenation itself


def test_one_rank_equals_execute_retain():
    from flock_amd.runtime import ExecutionContext
    table = make_table(0, TILE + 77, seed=5)
    got = exchange_once(1, [table], "s0")[0]

    def body(r, gpu, comm):
        p = ExecutionContext([producer_plan("s0")], gpu=gpu, generic_only=True)
        c = ExecutionContext([pc.scan(COLS).plan], gpu=gpu, generic_only=True)
        try:
            p.feed_data_sources([[[batch(table)]]])
            p.execute_retain()
            c.feed_from([p])
            return rows_of(c.execute()[0])
        finally:
            c.clean_data_sources(), p.clean_data_sources(), c.close(), p.close()
    assert got == run_ranks(1, body)[0] == table_rows(table)


@pytest.mark.parametrize("world", [2, 3])
def test_a_filter_directly_below_the_repartition(world):
    """the filter's row list is composed with the send order: an Int64 column, a validity column and Utf8 columns go through it"""
    cols = [("k64", "Int64"), ("f", "Float64"), ("s2", "Utf8"), ("src", "Int64")]
    node = pc.scan(cols)
    bound = 15 * (2**40 + 3) - 2**50          # (make_table: k64 takes 40 values; those above the 15th pass)
    plan = producer_plan("k64", cols, pc.filt(node, pc.binop(node.c("k64"), "Gt", pc.lit("Int64", bound))))
    tables = [make_table(r, 2 * TILE + 9, seed=6) for r in range(world)]
    got = exchange_once(world, tables, cols=cols, plan=plan)
    want = [row for t in tables for row in table_rows(t, cols) if row[0] is not None and row[0] > bound]
    assert want and multiset([row for g in got for row in g]) == multiset(want)
    check_placement(got, 0)
    check_order(got, 3)


def test_validity_on_one_rank_only_reaches_every_receiver():
    world = 3
    tables = [make_table(r, 4000, seed=7, nulls=0.3 if r == 1 else 0.0) for r in range(world)]
    got = exchange_once(world, tables, "k32")
    want = [row for t in tables for row in table_rows(t)]
    assert any(None in row for row in want)
    assert multiset([row for g in got for row in g]) == multiset(want)
    check_order(got)


def test_an_all_null_maximum_is_gathered_next_to_real_values():
    """MAX over no rows on rank 1 (one all-NULL row) next to the other ranks' maxima, gathered on rank 0"""
    world = 3
    cols = [("k64", "Int64"), ("src", "Int64")]
    part = pc.aggregate(pc.scan(cols), [], [("max", "k64"), ("max", "src")], single="Partial")
    tables = [make_table(r, 0 if r == 1 else 1000, seed=8, nulls=0.0) for r in range(world)]
    got = exchange_once(world, tables, cols=cols, gather_rank=0, plan=part.plan, consumer=pc.scan(part.cols).plan)
    assert got[1] == [] and got[2] == []
    assert got[0] == [(max(tables[0]["k64"]), max(tables[0]["src"])), (None, None), (max(tables[2]["k64"]), max(tables[2]["src"]))]


@pytest.mark.parametrize("world,target", [(2, 0), (3, 0), (3, 2)])
def test_gather_lands_everything_on_one_rank_in_rank_order(world, target):
    tables = [make_table(r, 3000 + r, seed=10) for r in range(world)]
    got = exchange_once(world, tables, "k64", gather_rank=target)
    for r in range(world):
        assert got[r] == ([row for t in tables for row in table_rows(t)] if r == target else [])


def test_a_rank_without_rows_takes_part_but_sends_nothing():
    world = 3
    tables = [make_table(r, 2000, seed=11) for r in range(world)]
    got = exchange_once(world, tables, "k64", gather_rank=0, no_rows=(1,))
    assert got[0] == table_rows(tables[0]) + table_rows(tables[2]) and got[1] == [] and got[2] == []
    got = exchange_once(world, tables, "k64", no_rows=(1,))
    assert multiset([row for g in got for row in g]) == multiset(table_rows(tables[0]) + table_rows(tables[2]))


def test_many_small_pieces_change_nothing():
    world = 3
    tables = [make_table(r, 3000, seed=12) for r in range(world)]
    assert exchange_once(world, tables, "ku", piece=4099) == exchange_once(world, tables, "ku")


def test_the_same_call_twice_gives_identical_batches():
    world = 3
    tables = [make_table(r, TILE + 5, seed=13) for r in range(world)]

    def body(r, gpu, comm):
        pair = Pair(gpu, producer_plan("kt"), pc.scan(COLS).plan)
        try:
            return pair.exchange(comm, tables[r]), pair.exchange(comm, tables[r])
        finally:
            pair.close()
    for first, second in run_ranks(world, body):
        assert first == second


def _code_of(fn):
    from flock_amd import FlockGpuError
    with pytest.raises(FlockGpuError) as e:
        fn()
    return e.value.code, str(e.value)


def test_argument_errors_come_back_before_any_collective():
    from flock_amd import _ffi
    world = 2
    tables = [make_table(r, 500, seed=14) for r in range(world)]
    hash_diff = pc.coalesce({"execution_plan": "repartition_exec", "input": pc.scan(COLS).plan, "partitioning": {"HashDiff": [[pc.scan(COLS).c("k32")], 4]}})

    def body(r, gpu, comm):
        from flock_amd.runtime import ExecutionContext
        pair = Pair(gpu, producer_plan("k64"), pc.scan(COLS).plan)
        bare = ExecutionContext([pc.scan(COLS).plan], gpu=gpu, generic_only=True)
        diff = ExecutionContext([hash_diff], gpu=gpu, generic_only=True)
        try:
            seen = []
            if r == 0:   # one rank alone: nothing of this reaches a collective, so the other rank need not make the same mistakes
                seen.append(_code_of(lambda: pair.p.exchange_retain(comm, world)))
                seen.append(_code_of(lambda: pair.p.plans[0].gpu._check(pair.p.plans[0]._lib.flockgpu_plan_exchange_retain(pair.p.plans[0].h, comm.h, -1, 6, None))))
                seen.append(_code_of(lambda: bare.exchange_retain(comm)))
                seen.append(_code_of(lambda: diff.exchange_retain(comm)))
            return seen, pair.exchange(comm, tables[r])
        finally:
            pair.close(), bare.close(), diff.close()
    out = run_ranks(world, body)
    codes = out[0][0]
    assert [c for c, _ in codes] == [_ffi.ERR_INVALID, _ffi.ERR_INVALID, _ffi.ERR_INVALID, _ffi.ERR_UNSUPPORTED]
    assert "HashDiff" in codes[3][1]
    assert multiset(out[0][1] + out[1][1]) == multiset(table_rows(tables[0]) + table_rows(tables[1]))


def test_a_failed_rank_fails_every_rank_and_the_communicators_go_on():
    from flock_amd import FlockGpuError, _ffi
    world = 3
    tables = [make_table(r, 1500, seed=15) for r in range(world)]

    def body(r, gpu, comm):
        pair = Pair(gpu, producer_plan("k64"), pc.scan(COLS).plan)
        try:
            if r == 1:
                comm.inject_failure(1)
            try:
                pair.exchange(comm, tables[r])
                code = _ffi.OK
            except FlockGpuError as e:
                code = e.code
            return code, pair.exchange(comm, tables[r])
        finally:
            pair.close()
    out = run_ranks(world, body)
    assert [c for c, _ in out] == [_ffi.ERR_PEER, _ffi.ERR_CAPACITY, _ffi.ERR_PEER]
    assert multiset([row for _, g in out for row in g]) == multiset([row for t in tables for row in table_rows(t)])


def test_ranks_with_different_schemas_are_all_refused():
    from flock_amd import FlockGpuError, _ffi
    world = 3
    other = [("k64", "Int64") if n == "k64" else (n, t) for n, t in COLS]
    other[4] = ("g", "Float64")          # the same column count and types, another name
    tables = [make_table(r, 800, seed=16) for r in range(world)]

    def body(r, gpu, comm):
        cols = other if r == 2 else COLS
        table = dict(tables[r], g=tables[r]["f"])
        pair = Pair(gpu, producer_plan("k64", cols), pc.scan(cols).plan)
        try:
            pair.exchange(comm, table, cols)
            return _ffi.OK
        except FlockGpuError as e:
            return e.code
        finally:
            pair.close()
    assert run_ranks(world, body) == [_ffi.ERR_INVALID] * world
