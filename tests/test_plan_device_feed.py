"""Device columns in and out of plans: flockgpu_plan_feed_columns / flockgpu_plan_result_columns (include/flockgpu_plan.h), `_Plan.feed_columns`,
`ExecutionContext.feed_device_sources` / `result_columns`, `flock_amd.nexmark.event_source`.

CPU: the declarations, the routing of device sources to leaves, the Python argument checks.  GPU: a plan fed the same rows from the host and from
device memory gives the same rows, and both give what tests/plan_interp.py computes -- over every boundary type, in one batch and in several, from
misaligned slices, with NULLs that are dropped, kept or absent, in place (borrow) and copied; the refusals by name and status; a retained result
through the device encoders against tests/text_encode_ref.py; text -> decode -> plan -> encode -> text without a host copy of a row."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pyarrow as pa
import pytest

import csv_ref
import device_feed_util as u
import plan_corpus as pc
import text_encode_ref as enc
from plan_interp import run_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = os.path.join(ROOT, "tests", "golden", "plans")
T = u.FLAG_TILE
FEED_ROWS = [0, 1, 5, T - 1, T, T + 1, 3 * T + 5]
BIG = 3 * T + 5


# ------------------------------------------------------------------ CPU
def test_both_symbols_are_declared_listed_and_exported():
    from flock_amd import _ffi, build
    build.build()
    lib = _ffi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flockgpu_plan.h")).read(), flags=re.S)
    for name in ("flockgpu_plan_feed_columns", "flockgpu_plan_result_columns"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _ffi.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"FLOCKGPU_FEED_BORROW\s*=\s*1u", header) and _ffi.FEED_BORROW == 1
    assert _ffi.SYMBOLS["flockgpu_plan_feed_columns"][1][2:] == [C.POINTER(_ffi.TextColumn), C.c_int32, C.c_int64, C.c_uint32]
    assert lib.flockgpu_abi_version() == _ffi.ABI_VERSION == 1          # an added entry point leaves the version where it was


class _FakePlan:
    """a plan as feed_device_sources sees it: leaves that need column names, feeds recorded"""
    def __init__(self, *needs):
        self.needs, self.inputs, self.fed = needs, ["" for _ in needs], []

    def matches(self, i, schema):
        return set(self.needs[i]) <= set(schema.names)

    def feed_columns(self, i, columns, valid=None, borrow=False):
        self.fed.append((i, [name for name, _, _ in columns], sorted(valid or {}), borrow))


def test_feed_device_sources_routes_every_source_to_every_leaf_it_covers():
    from flock_amd.runtime import ExecutionContext, _columns_schema
    ctx = ExecutionContext.__new__(ExecutionContext)
    one, two = _FakePlan(["auction", "price"], ["a_id"], ["auction"]), _FakePlan(["p_id", "name"], ["nothing_has_this"])
    ctx.plans, ctx._ring = [one, two], 0
    bid = ([("auction", "int32", None), ("price", "int32", None), ("b_date_time", "timestamp_ms", None)], {"price": None})
    person = ([("p_id", "int32", None), ("name", "utf8", None)], None)
    assert ctx.feed_device_sources([bid, person], borrow=True) == 3
    # the bid source feeds BOTH leaves that read bids (nothing moves when a device source is fed), no source covers a_id, the person source finds its leaf
    assert one.fed == [(0, ["auction", "price", "b_date_time"], ["price"], True), (2, ["auction", "price", "b_date_time"], ["price"], True)]
    assert two.fed == [(0, ["p_id", "name"], [], True)]
    schema = _columns_schema(bid[0])
    assert schema.names == ["auction", "price", "b_date_time"] and schema.field("b_date_time").type == pa.timestamp("ms")
    with pytest.raises(ValueError, match="unknown type"):
        _columns_schema([("x", "decimal", None)])
    ctx._ring = 4
    with pytest.raises(ValueError, match="ring"):
        ctx.feed_device_sources([bid])


def test_feed_columns_checks_its_arguments_before_any_call():
    import torch
    from flock_amd.engine import DeviceUtf8, GpuContext
    from flock_amd.runtime import _Plan
    plan = _Plan.__new__(_Plan)
    plan.gpu, plan._lib, plan.h, plan._fed, plan._base_fed = GpuContext.__new__(GpuContext), None, None, [], set()
    i32, i64, ok = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), torch.ones(4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="^feed_columns: column 'a': int32 does not take 8-byte"):
        plan.feed_columns(0, [("a", "int32", i64)])
    with pytest.raises(ValueError, match="timestamp_ms does not take 4-byte"):
        plan.feed_columns(0, [("a", "timestamp_ms", i32)])
    with pytest.raises(ValueError, match="^feed_columns: validity for unknown column"):      # (the caller fed a plan: the message says so)
        plan.feed_columns(0, [("a", "int32", i32)], {"b": ok})
    with pytest.raises(ValueError, match="has 3 rows"):
        plan.feed_columns(0, [("a", "int32", i32), ("s", "utf8", DeviceUtf8(torch.zeros(4, dtype=torch.int32), torch.zeros(16, dtype=torch.uint8)))])
    with pytest.raises(ValueError, match="validity of 'a' has 4 entries for 2 rows"):
        plan.feed_columns(0, [("a", "int32", i32[:2])], {"a": ok})
    with pytest.raises(ValueError, match="takes a DeviceUtf8"):
        plan.feed_columns(0, [("s", "utf8", i32)])
    assert plan._fed == []


def test_event_source_types_the_relation():
    from flock_amd.engine import Bids
    from flock_amd.nexmark import event_source
    cols, valid = event_source("bid", Bids(auction="A", price="P", b_date_time="T", rows=3))
    assert cols == [("auction", "int32", "A"), ("price", "int32", "P"), ("b_date_time", "timestamp_ms", "T")] and valid == {}
    cols, _ = event_source("auction", {"a_id": 1, "expires": 2, "a_date_time": 3, "item_name": 4, "extra": 5})
    assert cols == [("a_id", "int32", 1), ("item_name", "utf8", 4), ("a_date_time", "timestamp_ms", 3), ("expires", "timestamp_ms", 2)]
    with pytest.raises(ValueError):
        event_source("person", {})


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    c = GpuContext(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _tables(kind, n, seed=1):
    """the tables of plan `kind` in leaf order: `a` has n rows, `b` (a join's small side) 300"""
    _, prefixes, _ = u.plan_of(kind)
    return tuple(u.table("a", n, seed, **(u.PLAIN if kind == "filter_plain" else {})) if p == "a" else u.build_side() for p in prefixes)


@functools.lru_cache(maxsize=None)
def _want(kind, n, seed=1):
    plan, _, ordered = u.plan_of(kind)
    rows = u.norm(run_plan(plan, list(_tables(kind, n, seed)))[2])
    return rows if ordered else u.multiset(rows)


def _fed(gpu, kind, tables, how, generic_only=False, **kw):
    """the rows of plan `kind` with every table fed by `how(run, t, table)`"""
    plan, _, ordered = u.plan_of(kind)
    run = u.Run(gpu, plan, generic_only)
    try:
        for t, table in enumerate(tables):
            how(run, t, table)
        return run.rows(ordered)
    finally:
        run.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", FEED_ROWS)
@pytest.mark.parametrize("kind", u.KINDS)
def test_device_fed_equals_host_fed_equals_the_interpreter(gpu, kind, n):
    tables, want = _tables(kind, n), _want(kind, n)
    host = _fed(gpu, kind, tables, lambda run, t, table: run.host(t, table))
    dev = _fed(gpu, kind, tables, lambda run, t, table: run.device(t, table))
    assert host == want, (kind, n, "host-fed differs from the interpreter")
    assert dev == want, (kind, n, "device-fed differs")


BATCHINGS = {
    "one_call": [("d", 0, BIG)],
    "three_calls": [("d", 0, 1), ("d", 1, T), ("d", T, BIG)],                  # 1, 8191 and the rest: every later destination is misaligned
    "device_host_device": [("d", 0, 1), ("h", 1, T), ("d", T, BIG)],
    "host_device_host": [("h", 0, 1), ("d", 1, T), ("h", T, BIG)],
}


def _profiled(gpu, fn):
    """fn() with every launch named: (its result, the kernels that ran)"""
    gpu.profile_reset()
    gpu.profile(True)
    try:
        got = fn()
        return got, set(gpu.profile_read())
    finally:
        gpu.profile(False)


def _check_route(kind, ran):
    """filter_plain leaves no row out: Utf8 offsets land rebased by offsets_rebase_kernel straight from the source, and take_tail_kernel -- which only a
    feed that drops rows launches -- does not run; filter_project and the joins drop rows at the feed: census flags, row list, tail take"""
    if kind == "filter_plain":
        assert {"feed_census_kernel", "offsets_rebase_kernel"} <= ran and "take_tail_kernel" not in ran, sorted(ran)
    elif kind in ("filter_project", "join_inner", "join_semi"):
        assert {"feed_census_kernel", "take_tail_kernel", "offsets_rebase_kernel"} <= ran, sorted(ran)


@pytest.mark.gpu
@pytest.mark.parametrize("how", sorted(BATCHINGS))
@pytest.mark.parametrize("kind", ["filter_project", "filter_plain", "join_inner", "group_by"])
def test_batching_does_not_change_the_result(gpu, kind, how):
    def feed(run, t, table):
        n = len(next(iter(table.values())))
        for where, lo, hi in (BATCHINGS[how] if n == BIG else [("d", 0, n)]):
            (run.device if where == "d" else run.host)(t, table, lo, hi)
    got, ran = _profiled(gpu, lambda: _fed(gpu, kind, _tables(kind, BIG), feed))
    assert got == _want(kind, BIG), (kind, how)
    _check_route(kind, ran)


@pytest.mark.gpu
@pytest.mark.parametrize("borrow", [False, True])
@pytest.mark.parametrize("shift", [1, 3])
@pytest.mark.parametrize("kind", ["filter_project", "filter_plain", "join_inner"])
def test_sources_need_only_their_natural_alignment(gpu, kind, shift, borrow):
    """every column a [shift:] slice of a larger tensor, Utf8 offsets starting at 3: the same rows as from aligned copies; with borrow the library
    copies (nothing is 16-byte aligned) and the result is the same.  An odd first batch in front: the leaf's tail is misaligned and its byte cursors
    are not 0 when the slices arrive (filter_plain: offsets[0] != 0 through the plain rebased append, bytes copied from data + offsets[0])"""
    n, cut = T + 1, 7

    def feed(run, t, table):
        rows = len(next(iter(table.values())))
        if rows == n:
            run.device(t, table, 0, cut)
            run.device(t, table, cut, n, shift=shift, borrow=borrow)
        else:
            run.device(t, table, shift=shift, borrow=borrow)
    got, ran = _profiled(gpu, lambda: _fed(gpu, kind, _tables(kind, n), feed))
    assert got == _want(kind, n), (kind, shift, borrow)
    _check_route(kind, ran)


# ---- NULLs
def _host_batch_of(columns):
    """device columns (no NULLs) as a record batch"""
    arrs, names = [], []
    for name, t, col in columns:
        names.append(name)
        if t == "utf8":
            off, data = col.offsets.cpu().numpy(), col.data.cpu().numpy()
            arrs.append(pa.StringArray.from_buffers(len(off) - 1, pa.py_buffer(off.tobytes()), pa.py_buffer(data.tobytes())))
        else:
            a = pa.array(col.cpu().numpy())
            arrs.append(a.cast(pa.timestamp("ms")) if t == "timestamp_ms" else a)
    return pa.record_batch(arrs, names=names)


@pytest.mark.gpu
def test_all_ones_validity_keeps_the_fused_q3_path(gpu):
    """validity bytes that are all 1 on EVERY column (what the CSV decoder writes): no validity reaches the leaf, the plan flockgpu_plan_recognise
    numbers q3 still runs its fused pipeline"""
    import torch
    from flock_amd import NEXMarkSource, Window, _ffi
    from flock_amd.nexmark import event_source
    from flock_amd.runtime import ExecutionContext
    plan = open(os.path.join(PLANS, "q3.json")).read()
    q = C.c_int(0)
    assert _ffi.load().flockgpu_plan_recognise(plan.encode(), len(plan.encode()), C.byref(q)) == 0 and q.value == 3
    g = NEXMarkSource(2, 50_000, Window.element_wise(), seed=3).generate_data(gpu, relations=("auction", "person"))
    sources = []
    for relation, cols in (("auction", g.auctions), ("person", g.persons)):
        columns, _ = event_source(relation, cols)
        rows = columns[0][2].numel()
        sources.append((columns, {name: torch.ones(rows, dtype=torch.uint8, device=f"cuda:{gpu.device}") for name, _, _ in columns}))
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        gpu.profile_reset()
        gpu.profile(True)
        assert ctx.feed_device_sources(sources) == 2
        dev = u.multiset(u.norm(u.batch_rows(ctx.execute()[0])))
        ran = set(gpu.profile_read())
        gpu.profile(False)
        ctx.clean_data_sources()
        ctx.feed_data_sources([[[_host_batch_of(columns)]] for columns, _ in sources])
        host = u.multiset(u.norm(u.batch_rows(ctx.execute()[0])))
        ctx.clean_data_sources()
    finally:
        gpu.profile(False)
        ctx.close()
    assert "feed_census_kernel" in ran, sorted(ran)
    assert any(k.startswith("q3_") for k in ran), sorted(ran)
    assert len(dev) > 0 and dev == host


@pytest.mark.gpu
def test_all_ones_validity_on_a_join_key_leaves_the_join_running(gpu):
    n = T + 1
    tables = tuple({k: [0 if x is None else x for x in v] if k.endswith("_k") else v for k, v in t.items()} for t in _tables("join_inner", n))
    plan = u.plan_of("join_inner")[0]
    want = u.multiset(u.norm(run_plan(plan, list(tables))[2]))
    assert _fed(gpu, "join_inner", tables, lambda run, t, table: run.device(t, table, validity="always")) == want


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["join_inner", "join_semi", "filter_project"])
def test_nulls_in_a_droppable_key_drop_the_rows_the_host_feed_drops(gpu, kind):
    """p = 0.15 in the key column (device_feed_util.table), garbage in the NULL slots: the validity bytes decide.  The rows equal the host feed's (and
    the interpreter's), count and content; the rows are left out by the feed itself, through the row list and the tail take"""
    n = 2 * T + 77
    tables = _tables(kind, n)
    got, ran = _profiled(gpu, lambda: _fed(gpu, kind, tables, lambda run, t, table: run.device(t, table, validity="always", null_slot=7)))
    host = _fed(gpu, kind, tables, lambda run, t, table: run.host(t, table))
    assert len(got) == len(host) and got == host == _want(kind, n)
    _check_route(kind, ran)


# ---- what lies under a NULL (tests/null_poison.py, the far pool: type extremes, NaNs, texts that match, that do not parse and that are no UTF-8)
def _far(kind):
    return ("far", ("device_feed", u.KINDS.index(kind), 0))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, BIG])
@pytest.mark.parametrize("kind", u.KINDS)
def test_device_fed_and_host_fed_over_far_poison_equal_the_interpreter(gpu, kind, n):
    """test_device_fed_equals_host_fed_equals_the_interpreter with hostile values and bytes under every NULL, from the host and from the device"""
    tables, want = _tables(kind, n), _want(kind, n)
    assert any(v is None for t in tables for col in t.values() for v in col)
    host = _fed(gpu, kind, tables, lambda run, t, table: run.host(t, table, poison=_far(kind)))
    dev = _fed(gpu, kind, tables, lambda run, t, table: run.device(t, table, poison=_far(kind)))
    assert host == want, (kind, n, "host-fed differs from the interpreter")
    assert dev == want, (kind, n, "device-fed differs")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", u.KINDS)
def test_far_poison_under_the_nulls_of_a_droppable_key_drops_the_rows_the_host_feed_drops(gpu, kind):
    """test_nulls_in_a_droppable_key_... for every kind, in three calls (1, 8191 and the rest: every later destination misaligned): bytes under NULL
    Utf8 rows go through take_tail_kernel and offsets_rebase_kernel, a_s and a_s2 through one take of several Utf8 columns"""
    n = BIG
    tables = _tables(kind, n)

    def feed(run, t, table):
        rows = len(next(iter(table.values())))
        for _, lo, hi in (BATCHINGS["three_calls"] if rows == n else [("d", 0, rows)]):
            run.device(t, table, lo, hi, validity="always", poison=_far(kind))
    got, ran = _profiled(gpu, lambda: _fed(gpu, kind, tables, feed))
    host = _fed(gpu, kind, tables, lambda run, t, table: run.host(t, table))
    assert len(got) == len(host) and got == host == _want(kind, n)
    _check_route(kind, ran)


@pytest.mark.gpu
def test_borrowed_columns_over_far_poison_are_read_in_place(gpu):
    """filter_plain fed with borrow=True: the leaf reads the caller's tensors -- poisoned slots, bytes under NULL texts and all -- without a copy"""
    n = T + 16
    table = _tables("filter_plain", n)[0]
    plan = u.plan_of("filter_plain")[0]
    run = u.Run(gpu, plan)
    try:
        held, ran = _profiled(gpu, lambda: run.device(0, table, borrow=True, poison=_far("filter_plain")))
        assert "feed_census_kernel" in ran and not ran & {"offsets_rebase_kernel", "take_tail_kernel"}, sorted(ran)
        assert run.rows() == _want("filter_plain", n)
        assert any(None in r for r in _want("filter_plain", n))
        del held
    finally:
        run.close()


@pytest.mark.gpu
def test_validity_arrives_with_a_column_that_reaches_the_output(gpu):
    """a first batch without a NULL anywhere, then one with: the earlier rows are back-filled as valid"""
    n, cut = T + 300, 301
    full = _tables("filter_project", n)[0]
    clean = u.table("a", cut, 9, nulls={c: 0.0 for c in ("u", "t", "f", "s", "s2", "v", "i")}, key_nulls=0.0)
    table = {k: clean[k] + full[k][cut:] for k in full}
    table["a_id"] = list(range(n))
    plan = u.plan_of("filter_project")[0]
    want = u.multiset(u.norm(run_plan(plan, [table])[2]))
    assert any(None in r for r in want)

    def feed(run, t, tab):
        run.device(t, tab, 0, cut)
        run.device(t, tab, cut, n)
    assert _fed(gpu, "filter_project", (table,), feed) == want


@pytest.mark.gpu
def test_a_batch_whose_droppable_column_is_all_null_adds_no_rows(gpu):
    n = 700
    table = _tables("filter_project", n)[0]
    nothing = dict(u.table("a", T + 3, 4), a_g=[None] * (T + 3))      # the filter compares a_g: its NULL rows are left out at the feed
    plan = u.plan_of("filter_project")[0]

    def feed(run, t, tab):
        run.device(t, tab)
        run.device(t, nothing)
        run.device(t, tab, 0, 5)
    want = u.multiset(u.norm(run_plan(plan, [{k: table[k] + table[k][:5] for k in table}])[2]))
    assert _fed(gpu, "filter_project", (table,), feed) == want


# ---- borrow
@pytest.mark.gpu
def test_borrowed_columns_are_read_until_reset_and_not_after(gpu):
    """filter_plain's tables hold no NULL where the feed could drop a row, and device_source's unshifted tensors are 16-byte aligned: a borrow feed of
    an empty leaf is read IN PLACE (a_u, a_t, a_s and others hold NULLs: borrowed validity, too).  Seen two ways: no copy or rebase kernel runs, and a
    value overwritten in a borrowed tensor AFTER the feed shows in the result."""
    n, k = T + 16, 1001
    first, second = _tables("filter_plain", n)[0], u.table("a", n, 11, **u.PLAIN)
    plan = u.plan_of("filter_plain")[0]
    want = lambda table: u.multiset(u.norm(run_plan(plan, [table])[2]))
    assert any(None in r for r in want(first))
    run = u.Run(gpu, plan)
    try:
        (columns, valid), ran = _profiled(gpu, lambda: run.device(0, first, borrow=True))
        assert "feed_census_kernel" in ran and not ran & {"offsets_rebase_kernel", "take_tail_kernel"}, sorted(ran)
        assert run.rows() == want(first)
        assert run.rows() == want(first)                             # executed twice
        changed = dict(first, a_i=[None if v is None else 12345 for v in first["a_i"]])
        dict((name, col) for name, _, col in columns)["a_i"].fill_(12345)
        assert run.rows() == want(changed) != want(first)            # the leaf reads the caller's tensor, not a copy of it
        run.p.reset()
        for _, _, col in columns:                                    # the promise ended with the reset: the tensors may change
            for t in ((col.offsets, col.data) if hasattr(col, "offsets") else (col,)):
                t.zero_()
        for v in valid.values():
            v.zero_()
        run.device(0, second, borrow=True)
        assert run.rows() == want(second)
        # feeds behind columns that are read in place append: the leaf takes its own copy of the borrowed rows first -- a device feed, then a host feed
        run.p.reset()
        run.device(0, first, 0, k, borrow=True)                      # in place again (an empty leaf)
        _, ran = _profiled(gpu, lambda: run.device(0, first, k, T, borrow=True))     # a leaf that holds rows: a copy, also with borrow
        assert "offsets_rebase_kernel" in ran, sorted(ran)
        assert run.rows() == u.multiset(u.norm(run_plan(plan, [{c: v[:T] for c, v in first.items()}])[2]))
        run.host(0, first, T, n)
        assert run.rows() == want(first)
        # ... and a HOST feed directly behind borrowed columns
        run.p.reset()
        held = run.device(0, first, 0, k, borrow=True)
        run.host(0, first, k, n)
        assert run.rows() == want(first)
        del held
        # after a reset the leaf is its own again: an ordinary feed, nothing of the borrowed columns left
        run.p.reset()
        run.device(0, second)
        assert run.rows() == want(second)
    finally:
        run.close()


# ---- refusals
@pytest.mark.gpu
def test_refusals_name_what_is_wrong_and_leave_the_leaf_as_it_was(gpu):
    import torch
    from flock_amd import _ffi
    from flock_amd._ffi import FlockGpuError
    n = 1000
    table = _tables("filter_project", n)[0]
    plan = u.plan_of("filter_project")[0]
    run = u.Run(gpu, plan)
    try:
        run.p.ring_open(2)
        with pytest.raises(FlockGpuError, match="plan_feed_columns: .*flockgpu_plan_feed_pane") as e:
            run.device(0, table)
        assert e.value.code == _ffi.ERR_INVALID
        run.p.ring_close()
        with pytest.raises(FlockGpuError, match="plan_result_columns: .*no retained result") as e:
            run.p.result_columns()
        assert e.value.code == _ffi.ERR_INVALID
        run.device(0, table)
        before = run.rows()
        assert before == _want("filter_project", n)
        columns, valid = u.device_source(run.fields[0], table, device=f"cuda:{gpu.device}")
        with pytest.raises(FlockGpuError, match="plan_feed_columns: column 'a_k' missing from the fed schema") as e:
            run.p.feed_columns(0, [c for c in columns if c[0] != "a_k"], {k: v for k, v in valid.items() if k != "a_k"})
        assert e.value.code == _ffi.ERR_INVALID
        assert run.rows() == before
        wrong = [(name, "int64", col.to(dtype=torch.int64)) if name == "a_k" else (name, t, col) for name, t, col in columns]
        with pytest.raises(FlockGpuError, match="plan_feed_columns: column 'a_k' has Arrow format 'l', the plan scans Int32") as e:
            run.p.feed_columns(0, wrong, valid)
        assert e.value.code == _ffi.ERR_UNSUPPORTED
        assert run.rows() == before
        # 2^31 rows: decided from `rows` alone, before anything is allocated or launched (the descriptors name 1000-row tensors)
        spec, _, keep = gpu._text_columns(columns, valid)
        gpu.profile_reset()
        gpu.profile(True)
        rc = run.p._lib.flockgpu_plan_feed_columns(run.p.h, run.leaf[0], spec, len(columns), 2**31, 0)
        ran = gpu.profile_read()
        gpu.profile(False)
        assert rc == _ffi.ERR_UNSUPPORTED and "2^31 rows" in gpu._lib.flockgpu_last_error(gpu._h).decode() and not ran, ran
        del keep
        assert run.rows() == before
        # the result view: capacity too small, *n_cols still set
        run.p.execute_retain()
        out, n_cols, rows = (_ffi.TextColumn * 2)(), C.c_int32(0), C.c_int64(-1)
        rc = run.p._lib.flockgpu_plan_result_columns(run.p.h, out, 2, C.byref(n_cols), C.byref(rows))
        assert rc == _ffi.ERR_INVALID and n_cols.value == 9 and "room for 2 columns" in gpu._lib.flockgpu_last_error(gpu._h).decode()
        assert run.rows() == before
    finally:
        gpu.profile(False)
        run.close()


# ---- result view
_ENC = {"Int32": "int32", "Int64": "int64", "UInt64": "uint64", "Utf8": "utf8"}


def _reference_columns(names, types, rows):
    """(names, types, rows) of the interpreter or of an exported batch -> text_encode_ref's columns and validity"""
    columns, valid = [], {}
    for c, (name, t) in enumerate(zip(names, types)):
        vals = [r[c] for r in rows]
        kind = "timestamp_ms" if isinstance(t, dict) else _ENC[t]
        ok = np.array([v is not None for v in vals], np.uint8)
        if not ok.all():
            valid[name] = ok
        if kind == "utf8":
            columns.append((name, kind, enc.utf8_of([b"" if v is None else (v if isinstance(v, bytes) else v.encode()) for v in vals])))
        else:
            columns.append((name, kind, np.array([0 if v is None else v for v in vals], dtype=np.uint64 if kind == "uint64" else np.int64)))
    return columns, valid


def _types_of(schema):
    names = {pa.int32(): "Int32", pa.int64(): "Int64", pa.uint64(): "UInt64", pa.string(): "Utf8"}
    return [pc.TS if pa.types.is_timestamp(f.type) else names[f.type] for f in schema]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["all_null", "validity"])
def test_a_retained_result_goes_through_the_device_encoders(gpu, case):
    a = pc.scan(pc.table_cols("a"))
    if case == "all_null":     # MAX / MIN / SUM over no rows: one row of NULLs beside a count of 0
        plan, table = pc.aggregate(a, [], [("count", None), ("max", "a_u"), ("min", "a_i"), ("sum", "a_v")]).plan, u.table("a", 0, 1)
    else:
        node = pc.keep(pc.filt(a, pc.binop(a.c("a_g"), "Lt", pc.lit("Int32", 3))), ["a_id", "a_k", "a_u", "a_t", "a_s", "a_s2", "a_i"])
        plan, table = node.plan, u.table("a", T + 9, 2)
    run = u.Run(gpu, plan)
    try:
        run.device(0, table)
        rb = run.p.execute()
        rows_ref = u.batch_rows([rb])
        columns_ref, valid_ref = _reference_columns(rb.schema.names, _types_of(rb.schema), rows_ref)
        assert valid_ref and len(rows_ref) > 0 and (case != "all_null" or len(rows_ref) == 1)
        assert run.p.execute_retain() == len(rows_ref)
        columns, valid, rows = run.ctx.result_columns()
        assert rows == len(rows_ref) and [(n, t) for n, t, _ in columns] == [(n, t) for n, t, _ in columns_ref]
        # (a column may carry validity bytes that are all 1 -- an aggregate's outputs do: the texts below decide what is NULL)
        assert set(valid_ref) <= set(valid) and all(bool(valid[name].all()) for name in set(valid) - set(valid_ref))
        assert bytes(gpu.csv_encode(columns, valid).cpu().numpy()) == enc.csv_text(columns_ref, valid_ref)
        assert bytes(gpu.json_lines_encode(columns, valid).cpu().numpy()) == enc.json_lines(columns_ref, valid_ref)
    finally:
        run.close()


# ---- text -> decode -> plan -> encode -> text
AUCTION = [("a_id", "Int32"), ("item_name", "Utf8"), ("description", "Utf8"), ("initial_bid", "Int32"), ("reserve", "Int32"), ("a_date_time", "ts"),
           ("expires", "ts"), ("seller", "Int32"), ("category", "Int32")]
BID = [("auction", "Int32"), ("bidder", "Int32"), ("price", "Int32"), ("b_date_time", "ts")]
_CSV = {"Int32": "int32", "Utf8": "utf8", "ts": "timestamp_ms"}


def _filter_group_sort(cols, where, key, aggs):
    s = pc.scan(cols)
    node = pc.aggregate(pc.filt(s, where(s)), [key], aggs)
    return pc.sort(node, [(key, False, False)]).plan


def _text_tensor(gpu, text):
    import torch
    return torch.from_numpy(np.frombuffer(text + b"\0" * (-len(text) % 16), np.uint8).copy()).to(f"cuda:{gpu.device}")[:len(text)]


@pytest.mark.gpu
def test_csv_text_to_plan_to_csv_text_without_a_host_copy_of_a_row(gpu):
    from flock_amd.runtime import ExecutionContext
    n, r = 20_000, np.random.default_rng(20)
    names = [b"plain", b'with "quotes"', b"comma, inside", b"", b"line\nbreak", "été".encode()]
    t0 = 1_600_000_000_000
    source = [("a_id", "int32", np.arange(1000, 1000 + n, dtype=np.int32)),
              ("item_name", "utf8", enc.utf8_of([names[int(x)] for x in r.integers(0, len(names), n)])),
              ("description", "utf8", enc.utf8_of([b"d" * int(x) for x in r.integers(0, 80, n)])),
              ("initial_bid", "int32", r.integers(1, 1000, n).astype(np.int32)),
              ("reserve", "int32", r.integers(1, 5000, n).astype(np.int32)),
              ("a_date_time", "timestamp_ms", t0 + np.arange(n, dtype=np.int64) * 997),
              ("expires", "timestamp_ms", t0 + np.arange(n, dtype=np.int64) * 997 + r.integers(1000, 10**7, n)),
              ("seller", "int32", r.integers(1000, 1400, n).astype(np.int32)),
              ("category", "int32", r.integers(10, 15, n).astype(np.int32))]
    holes = {"reserve": (r.random(n) >= 0.1).astype(np.uint8), "category": (r.random(n) >= 0.05).astype(np.uint8), "initial_bid": (r.random(n) >= 0.02).astype(np.uint8)}
    text = enc.csv_text(source, holes)
    assert b'""' in text and b",," in text
    fields = [(name, _CSV[t]) for name, t in AUCTION]
    cols, valid, rows = csv_ref.decode(text, fields)
    assert rows == n
    table = {}
    for name, t in fields:
        if t == "utf8":
            table[name] = [s.decode() for s in enc.strings_of(cols[name])]
        else:
            table[name] = [int(v) if ok else None for v, ok in zip(cols[name].tolist(), valid[name].tolist())]
    plan = _filter_group_sort(AUCTION, lambda s: pc.binop(s.c("initial_bid"), "Gt", pc.lit("Int32", 200)), "category",
                              [("count", None), ("sum", "reserve"), ("max", "expires"), ("min", "seller")])
    want = enc.csv_text(*_reference_columns(*run_plan(plan, [table])))
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        d_cols, d_valid, d_rows = gpu.csv_decode(_text_tensor(gpu, text), fields, borrow=True)
        assert d_rows == n and sorted(d_valid) == ["category", "initial_bid", "reserve"]
        assert ctx.feed_device_sources([([(name, t, d_cols[name]) for name, t in fields], d_valid)]) == 1
        ctx.execute_retain()
        got = bytes(gpu.csv_encode(*ctx.result_columns()[:2]).cpu().numpy())
        ctx.clean_data_sources()
    finally:
        ctx.close()
    assert got == want and want.count(b"\n") == 7          # the header, five categories, the group of the NULL category


@pytest.mark.gpu
def test_event_json_to_plan_to_json_lines(gpu):
    import torch
    from flock_amd.nexmark import columns_to_event_bytes, event_bytes_to_columns, event_source
    from flock_amd.runtime import ExecutionContext
    n, r = 20_000, np.random.default_rng(21)
    bids = {"auction": r.integers(1000, 1040, n).astype(np.int32), "bidder": r.integers(1, 10**6, n).astype(np.int32),
            "price": r.integers(1, 10**4, n).astype(np.int32), "b_date_time": 1_600_000_000_000 + np.arange(n, dtype=np.int64) * 13}
    table = {k: v.tolist() for k, v in bids.items()}
    plan = _filter_group_sort(BID, lambda s: pc.binop(pc.binop(s.c("auction"), "Modulo", pc.lit("Int32", 3)), "Eq", pc.lit("Int32", 0)), "auction",
                              [("count", None), ("max", "price"), ("max", "b_date_time")])
    want = enc.json_lines(*_reference_columns(*run_plan(plan, [table])))
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        text = columns_to_event_bytes(gpu, "bid", {k: torch.from_numpy(v).to(f"cuda:{gpu.device}") for k, v in bids.items()})
        cols, rows = event_bytes_to_columns(gpu, text, "bid")
        assert rows == n
        assert ctx.feed_device_sources([event_source("bid", cols)]) == 1
        ctx.execute_retain()
        got = bytes(gpu.json_lines_encode(*ctx.result_columns()[:2]).cpu().numpy())
        ctx.clean_data_sources()
    finally:
        ctx.close()
    assert got == want and want.count(b"\n") == 13


# ---- staged
@pytest.mark.gpu
def test_a_staged_run_over_device_fed_relations_equals_the_whole_plan(gpu):
    from flock_amd import NEXMarkSource, Window
    from flock_amd import stages as S
    from flock_amd.nexmark import event_source
    from flock_amd.runtime import ExecutionContext
    plan = json.load(open(os.path.join(PLANS, "q3.json")))
    g = NEXMarkSource(2, 50_000, Window.element_wise(), seed=7).generate_data(gpu, relations=("auction", "person"))
    relations = {"auction": event_source("auction", g.auctions), "person": event_source("person", g.persons)}
    ctx = ExecutionContext([plan], gpu=gpu)
    try:
        assert ctx.feed_device_sources(list(relations.values())) == 2
        whole = u.multiset(u.norm(u.batch_rows(ctx.execute()[0])))
        ctx.clean_data_sources()
    finally:
        ctx.close()
    staged = S.StagedRun(gpu, S.build_query_dag(plan), instances=1, on_device=True)
    try:
        out = staged.run(relations)
    finally:
        staged.close()
    out = out if isinstance(out, list) else [out]
    assert len(whole) > 0 and u.multiset(u.norm(u.batch_rows(out))) == whole
    host_staged = S.StagedRun(gpu, S.build_query_dag(plan), instances=1)      # device sources take the on-device hand-over: anything else says so
    try:
        with pytest.raises(ValueError, match="on_device"):
            host_staged.run(relations)
    finally:
        host_staged.close()
