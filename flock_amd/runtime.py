"""`ExecutionContext` -- the GPU twin of flock/src/runtime/context.rs, over the plan-level C ABI.

Same surface and argument meaning as the reference:

    ctx = ExecutionContext(plans=[plan_json, ...], name="SX72HzqFz1Qij4bP-00-00")
    ctx.feed_data_sources(sources)      # sources[relation][partition][batch]   (context.rs:257-325)
    batches = ctx.execute()             # -> [plan][batch]                      (context.rs:172-191)
    parts = ctx.execute_partitioned()   # -> [plan][partition][batch]           (context.rs:197-216)
    ctx.clean_data_sources()            #                                       (context.rs:227-254)

`collect(ctx, streams)` restates `actor::collect` (flock-function/src/aws/actor.rs:54-79); `explain(plan)` shows the
operator tree the engine built and what executes each node.  Plans are the
serde_json text of the reference's physical plans; data are pyarrow RecordBatches handed over through the
Arrow C Data Interface (what arrow-rs would export as FFI_ArrowArray).  A plan the engine does not recognise
raises `FlockGpuError` with status FLOCKGPU_ERR_UNSUPPORTED (the reference host would keep DataFusion for it).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import json
from typing import List, Optional, Sequence, Union

from . import _ffi
from ._ffi import FlockGpuError
from .engine import DeviceUtf8, GpuContext

_ARROW_SCHEMA_BYTES, _ARROW_ARRAY_BYTES = 72, 80


def _pa():
    import pyarrow as pa
    return pa


# An exported ArrowArray / ArrowSchema is released by calling the `release` callback stored inside it (Arrow C Data Interface:
# offset 64 of the 80-byte ArrowArray, offset 56 of the 72-byte ArrowSchema).  Re-importing the struct into pyarrow releases it,
# too, but builds a Python object per column on the way -- per fed batch, 52 batches per window at the reference's granule.
_RELEASE = C.CFUNCTYPE(None, C.c_void_p)


def _release(addr: int, offset: int):
    fn = C.c_void_p.from_address(addr + offset).value
    if fn:
        _RELEASE(fn)(addr)


@contextlib.contextmanager
def _exported(batches):
    """`batches` (not empty) and their schema as Arrow C structs: (schema pointer, array of batch pointers).  The library only borrows
    the batches -- the caller keeps them alive -- so the exported structs are handed back as the block ends."""
    sbuf = C.create_string_buffer(_ARROW_SCHEMA_BYTES)
    batches[0].schema._export_to_c(C.addressof(sbuf))
    abufs = [C.create_string_buffer(_ARROW_ARRAY_BYTES) for _ in batches]
    for b, ab in zip(batches, abufs):
        b._export_to_c(C.addressof(ab))
    try:
        yield C.cast(sbuf, C.c_void_p), (C.c_void_p * len(batches))(*[C.addressof(ab) for ab in abufs])
    finally:
        for ab in abufs:
            _release(C.addressof(ab), 64)
        _release(C.addressof(sbuf), 56)


def _columns_schema(columns):
    """The Arrow schema [(name, type, column)] stands for (the type names of csv_decode / csv_encode)."""
    pa = _pa()
    types = {"int32": pa.int32(), "int64": pa.int64(), "uint64": pa.uint64(), "float64": pa.float64(), "timestamp_ms": pa.timestamp("ms"),
             "utf8": pa.utf8()}
    for name, t, _ in columns:
        if t not in types:
            raise ValueError(f"device source: column {name!r}: unknown type {t!r}")
    return pa.schema([(name, types[t]) for name, t, _ in columns])


class _Plan:
    def __init__(self, gpu: GpuContext, text: str, generic_only: bool = False):
        self.gpu, self.text = gpu, text
        self._lib = _ffi.load()
        raw = text.encode()
        h = C.c_void_p()
        gpu._check(self._lib.flockgpu_plan_create_ex(gpu._h, raw, len(raw), _ffi.PLAN_GENERIC_ONLY if generic_only else 0, C.byref(h)))
        self.h = h
        self.query = self._lib.flockgpu_plan_query(h)
        self.inputs = [self._lib.flockgpu_plan_input_name(h, i).decode() for i in range(self._lib.flockgpu_plan_num_inputs(h))]
        self.description = self._lib.flockgpu_plan_description(h).decode()
        self.is_shuffling = bool(self._lib.flockgpu_plan_is_shuffling(h))
        self.partitions = self._lib.flockgpu_plan_output_partitions(h)
        self._fed = []   # the library borrows fed buffers until execute / reset returns (flockgpu_plan.h)
        self._base_fed = set()   # leaves that `feed` / `feed_shared` gave a base relation since the last reset: `feed_from` passes them by
        self._match_cache = {}

    def close(self):
        if self.h:
            self._lib.flockgpu_plan_destroy(self.h)
            self.h = None

    def matches(self, i: int, schema) -> bool:
        try:   # a function instance sees the same few schemas on every invocation: ask the library once per (leaf, schema)
            hit = self._match_cache.get((i, schema))
        except TypeError:
            hit = None
        if hit is not None:
            return hit
        ok = self._matches_uncached(i, schema)
        try:
            self._match_cache[(i, schema)] = ok
        except TypeError:
            pass
        return ok

    def _matches_uncached(self, i: int, schema) -> bool:
        buf = C.create_string_buffer(_ARROW_SCHEMA_BYTES)
        schema._export_to_c(C.addressof(buf))
        ok = self._lib.flockgpu_plan_input_matches(self.h, i, C.cast(buf, C.c_void_p)) == 1
        _pa().Schema._import_from_c(C.addressof(buf))  # takes ownership back and releases
        return ok

    def feed(self, i: int, batches: Sequence, pane: Optional[int] = None):
        """feed_data_sources for leaf i; with `pane` the batches are pane `pane` of the plan's device-side window ring
        (flockgpu_plan_feed_pane: only the new pane crosses PCIe, the ring keeps the others)."""
        pa = _pa()
        batches = [b for b in batches if b is not None]
        if not batches:
            if pane is not None:   # an empty pane still advances the ring
                self.gpu._check(self._lib.flockgpu_plan_feed_pane(self.h, i, pane, None, None, 0))
            return
        self._fed.append(batches)
        with _exported(batches) as (schema, ptrs):
            if pane is None:
                rc = self._lib.flockgpu_plan_feed(self.h, i, schema, ptrs, len(batches))
            else:
                rc = self._lib.flockgpu_plan_feed_pane(self.h, i, pane, schema, ptrs, len(batches))
        self.gpu._check(rc)
        self._base_fed.add(i)

    def prefetch(self, i: int, batches: Sequence, pane: int) -> bool:
        """The NEXT pane's batches of leaf i start moving to the device now, beside whatever the plan is executing
        (flockgpu_plan_prefetch_pane); `feed_prefetched(i, pane)` appends them when the pane's turn has come.  False -- nothing was
        started -- when the pane holds what a prefetch does not take (NULLs): feed it the ordinary way then."""
        batches = [b for b in batches if b is not None]
        if not batches:
            return False
        with _exported(batches) as (schema, ptrs):
            rc = self._lib.flockgpu_plan_prefetch_pane(self.h, i, pane, schema, ptrs, len(batches))
        if rc == _ffi.ERR_UNSUPPORTED:
            return False
        self.gpu._check(rc)
        self._prefetched = batches     # borrowed until the reset after the pane's feed
        return True

    def feed_prefetched(self, i: int, pane: int):
        self.gpu._check(self._lib.flockgpu_plan_feed_pane(self.h, i, pane, None, None, 0))
        self._fed.append(getattr(self, "_prefetched", None))
        self._prefetched = None

    def feed_shared(self, i: int, donor: "_Plan", donor_input: int) -> bool:
        """Leaf i reads the relation `donor`'s leaf was fed, in place (flockgpu_plan_feed_shared).  False -- and nothing changed --
        when the donor does not hold what this plan reads."""
        rc = self._lib.flockgpu_plan_feed_shared(self.h, i, donor.h, donor_input)
        if rc == _ffi.ERR_UNSUPPORTED:
            return False
        self.gpu._check(rc)
        self._base_fed.add(i)
        return True

    def execute_retain(self) -> int:
        """Runs the plan and leaves the result on the device for `feed_from` of the plans that consume it; returns its row count."""
        rows = C.c_int64(0)
        self.gpu._check(self._lib.flockgpu_plan_execute_retain(self.h, C.byref(rows)))
        return rows.value

    def exchange_retain(self, comm, gather_rank: int = -1, no_rows: bool = False) -> int:
        """The collective twin of `execute_retain` (flockgpu_plan_exchange_retain): every rank of `comm` calls it on its instance of the
        same stage plan; the result is hash-partitioned over the ranks by the root's hash keys -- or, `gather_rank >= 0`, sent whole to
        that rank -- and what THIS rank receives stays on the device for `feed_from`.  `no_rows`: the plan is not executed, the rank only
        takes part in the collectives (it hosts no instance of this stage).  Returns the rows received."""
        rows = C.c_int64(0)
        self.gpu._check(self._lib.flockgpu_plan_exchange_retain(self.h, comm.h, int(gather_rank), _ffi.EXCHANGE_NO_ROWS if no_rows else 0, C.byref(rows)))
        return rows.value

    def feed_from(self, i: int, producer: "_Plan") -> bool:
        """Leaf i reads `producer`'s retained result in place.  False -- nothing changed -- when that result lacks a column the leaf reads."""
        rc = self._lib.flockgpu_plan_feed_from(self.h, i, producer.h)
        if rc == _ffi.ERR_UNSUPPORTED:
            return False
        self.gpu._check(rc)
        return True

    def feed_columns(self, i: int, columns, valid=None, borrow: bool = False, pane: Optional[int] = None):
        """`feed` for rows that already lie in device memory (flockgpu_plan_feed_columns): `columns` = [(name, "int32" | "int64" | "uint64" |
        "float64" | "timestamp_ms" | "utf8", tensor | DeviceUtf8)] and `valid` = {name: uint8 tensor, 1 = not NULL}, csv_encode's argument
        shape -- what csv_decode, json_lines_decode and the device generator leave in HBM.  Columns are matched to the leaf by name, extra
        ones are ignored; the rows append behind what the leaf holds.  `borrow`: the tensors stay as they are until `reset`, and the library
        may read them in place instead of copying (it decides; the result is the same).  Either way this object holds the tensors until
        `reset`: the library reads them on its own stream.  With `pane` the rows are pane `pane` of the plan's device-side window ring
        (flockgpu_plan_feed_pane_columns; no columns: an empty pane, which still advances the ring); a ring outlives the reset that ends a
        borrow, so `borrow` does not go with it."""
        if pane is not None and borrow:
            raise ValueError("feed_columns: `borrow` does not go with `pane` (the ring outlives the reset that ends a borrow)")
        spec, rows, keep = self.gpu._text_columns(columns, valid, who="feed_columns")
        if pane is None:
            rc = self._lib.flockgpu_plan_feed_columns(self.h, i, spec, len(columns), rows, _ffi.FEED_BORROW if borrow else 0)
        else:
            rc = self._lib.flockgpu_plan_feed_pane_columns(self.h, i, pane, spec if columns else None, len(columns), rows, 0)
        self.gpu._check(rc)
        self._fed.append(keep)
        self._base_fed.add(i)

    def result_columns(self):
        """The result `execute_retain` / `exchange_retain` left on the device, as (columns, valid, rows) in `feed_columns`' and csv_encode's
        shape: views of the plan's own buffers (flockgpu_plan_result_columns), valid until the plan's next execute, feed or reset."""
        import torch
        cap = 64
        while True:
            spec = (_ffi.TextColumn * cap)()
            n, rows = C.c_int32(0), C.c_int64(0)
            rc = self._lib.flockgpu_plan_result_columns(self.h, spec, cap, C.byref(n), C.byref(rows))
            if rc == _ffi.ERR_INVALID and n.value > cap:
                cap = n.value
                continue
            self.gpu._check(rc)
            break
        names = {_ffi.TEXT_INT32: "int32", _ffi.TEXT_INT64: "int64", _ffi.TEXT_UINT64: "uint64", _ffi.TEXT_FLOAT64: "float64",
                 _ffi.TEXT_TIMESTAMP_MS: "timestamp_ms", _ffi.TEXT_UTF8: "utf8"}
        view, r = self.gpu._device_view, rows.value
        columns, valid = [], {}
        utf8 = [c for c in spec[:n.value] if c.type == _ffi.TEXT_UTF8]
        ends = {}
        if utf8 and r:   # a Utf8 column's byte count is its last offset: read once for all of them
            self.gpu.synchronize()
            ends = {c.name: int(view(c.utf8.offsets + 4 * r, 1, torch.int32).cpu()[0]) for c in utf8}
        for c in spec[:n.value]:
            name, t = c.name.decode(), names[c.type]
            if t == "utf8":
                col = DeviceUtf8(view(c.utf8.offsets, r + 1, torch.int32), view(c.utf8.data, ends.get(c.name, 0), torch.uint8))
            elif t == "int32":
                col = view(c.values, r, torch.int32)
            elif t == "float64":
                col = view(c.values, r, torch.int64).view(torch.float64)
            else:
                col = view(c.values, r, torch.int64)
            columns.append((name, t, col))
            if c.valid:
                valid[name] = view(c.valid, r, torch.uint8)
        return columns, valid, r

    def execute(self):
        pa = _pa()
        sbuf = C.create_string_buffer(_ARROW_SCHEMA_BYTES)
        abuf = C.create_string_buffer(_ARROW_ARRAY_BYTES)
        self.gpu._check(self._lib.flockgpu_plan_execute(self.h, C.cast(sbuf, C.c_void_p), C.cast(abuf, C.c_void_p)))
        return pa.RecordBatch._import_from_c(C.addressof(abuf), C.addressof(sbuf))

    def execute_partitioned(self):
        """[partition] -> RecordBatch: the plan's hash partitions when it is a shuffling stage, else one batch."""
        pa = _pa()
        cap = max(self.partitions, 1)
        sbuf = C.create_string_buffer(_ARROW_SCHEMA_BYTES)
        abufs = C.create_string_buffer(_ARROW_ARRAY_BYTES * cap)
        n = C.c_int(0)
        self.gpu._check(self._lib.flockgpu_plan_execute_partitioned(self.h, C.cast(sbuf, C.c_void_p), C.cast(abufs, C.c_void_p), cap, C.byref(n)))
        schema = pa.Schema._import_from_c(C.addressof(sbuf))
        return [pa.RecordBatch._import_from_c(C.addressof(abufs) + p * _ARROW_ARRAY_BYTES, schema) for p in range(n.value)]

    def reset(self):
        self.gpu._check(self._lib.flockgpu_plan_reset(self.h))
        self._fed = []
        self._base_fed = set()

    # -- asynchronous execute (flockgpu_plan_execute_async / flockgpu_plan_wait)
    def execute_async(self, partitioned: bool = False):
        self.gpu._check(self._lib.flockgpu_plan_execute_async(self.h, 1 if partitioned else 0))
        self._async_partitioned = partitioned

    def wait(self):
        """The batches of the execute started by `execute_async`: one RecordBatch, or [partition] -> RecordBatch."""
        pa = _pa()
        cap = max(self.partitions, 1)
        sbuf = C.create_string_buffer(_ARROW_SCHEMA_BYTES)
        abufs = C.create_string_buffer(_ARROW_ARRAY_BYTES * cap)
        n = C.c_int(0)
        self.gpu._check(self._lib.flockgpu_plan_wait(self.h, C.cast(sbuf, C.c_void_p), C.cast(abufs, C.c_void_p), cap, C.byref(n)))
        schema = pa.Schema._import_from_c(C.addressof(sbuf))
        out = [pa.RecordBatch._import_from_c(C.addressof(abufs) + p * _ARROW_ARRAY_BYTES, schema) for p in range(n.value)]
        return out if self._async_partitioned else out[0]

    # -- device-side pane ring (flockgpu_plan_ring_*)
    def ring_open(self, panes_per_window: int):
        self.gpu._check(self._lib.flockgpu_plan_ring_open(self.h, panes_per_window))

    def ring_close(self):
        self.gpu._check(self._lib.flockgpu_plan_ring_close(self.h))
        self._fed = []

    def ring_state(self):
        first, n, ppw = C.c_int64(0), C.c_int(0), C.c_int(0)
        self.gpu._check(self._lib.flockgpu_plan_ring_state(self.h, C.byref(first), C.byref(n), C.byref(ppw)))
        return first.value, n.value, ppw.value


class ExecutionContext:
    """Cloud execution context of one function: plans + name (context.rs:103-131)."""

    def __init__(self, plans: Sequence[Union[str, dict]], name: str = "flockgpu-00", gpu: Optional[GpuContext] = None,
                 device: int = 0, generic_only: bool = False, gpus: Optional[Sequence[GpuContext]] = None):
        """`gpus`: one GpuContext (stream) per plan -- what `execute` needs to run the plans side by side like the reference's tokio
        tasks; with a single `gpu` the plans share its stream and run one after the other.  `generic_only`: no fused pipeline."""
        self.name = name
        self._gpu = gpu or (gpus[0] if gpus else GpuContext(device))
        self._owns_gpu = gpu is None and not gpus
        ctxs = list(gpus) if gpus else [self._gpu] * len(plans)
        if len(ctxs) != len(plans):
            raise ValueError("ExecutionContext: one GpuContext per plan")
        self.plans: List[_Plan] = [_Plan(g, p if isinstance(p, str) else json.dumps(p), generic_only) for g, p in zip(ctxs, plans)]
        self._ring = 0

    # -- hopping windows: the device-side pane ring (flockgpu_plan.h; reference: window/hopping.rs:52-74 re-sends every window whole)
    def open_window_ring(self, panes_per_window: int):
        """From now on `feed_data_sources(sources, pane=p)` feeds ONE pane (hop seconds of events); execute() runs the window of the
        last `panes_per_window` panes, clean_data_sources() retires the oldest."""
        for plan in self.plans:
            plan.ring_open(panes_per_window)
        self._ring = panes_per_window

    def close_window_ring(self):
        for plan in self.plans:
            plan.ring_close()
            plan._prefetched = None
        self._ring = 0
        self._pre = None

    # -- context.rs:257-325
    def feed_data_sources(self, sources, pane: Optional[int] = None):
        """`sources[relation][partition][batch]`.  Every plan leaf takes the first remaining source whose first
        non-empty batch matches the leaf's columns by name (compare_schema, context.rs:402-416); a leaf without
        a match stays an empty relation (context.rs:305-314).  `pane`: see open_window_ring."""
        if (pane is None) != (not self._ring):
            raise ValueError("feed_data_sources: `pane` goes with an open window ring")
        pre = getattr(self, "_pre", None)
        if sources is None:   # the pane prefetch_data_sources announced
            if pre is None or pre["pane"] != pane:
                raise ValueError("feed_data_sources(None, pane): no prefetch for this pane")
            self._pre = None   # (whatever happens below, the announcement is used up)
            touched = set()
            for plan, i, batches in pre["later"]:
                plan.feed(i, batches, pane)
                touched.add(id(plan))
            for plan, i in pre["moving"]:
                plan.feed_prefetched(i, pane)
                touched.add(id(plan))
            for plan in self.plans:
                if id(plan) not in touched and plan.inputs:
                    plan.feed(0, [], pane)
            return
        if pre is not None:
            raise ValueError("feed_data_sources: pane %d was prefetched -- feed it with sources=None first" % pre["pane"])
        fed = set()
        for plan, i, batches in self._leaf_sources(sources):
            plan.feed(i, batches, pane)
            fed.add(id(plan))
        if pane is not None:
            for plan in self.plans:
                if id(plan) not in fed and plan.inputs:   # nothing arrived in this pane: the ring still advances
                    plan.feed(0, [], pane)

    def _leaf_sources(self, sources):
        """(plan, leaf, batches) for every plan leaf that finds a source: the first remaining source whose first batch matches the
        leaf's columns by name.  A source goes to one leaf only."""
        sources = [list(s) for s in sources]
        for plan in self.plans:
            for i in range(len(plan.inputs)):
                for si, partitions in enumerate(sources):
                    first = next((b for part in partitions for b in part), None)
                    if first is not None and plan.matches(i, first.schema):
                        yield plan, i, [b for part in sources.pop(si) for b in part]
                        break

    # -- device columns in and out (flockgpu_plan_feed_columns / flockgpu_plan_result_columns)
    def _device_leaf_sources(self, sources):
        """(plan, leaf, index into `sources`) for every plan leaf that finds a device source: the first source whose column names cover what
        the leaf reads -- feed_data_sources' matching (flockgpu_plan_input_matches) on a schema made of the names and types.  Nothing moves
        when a device source is fed, so one source may serve several leaves (q5's plan scans `bid` twice)."""
        schemas = [_columns_schema(columns) for columns, _ in sources]
        for plan in self.plans:
            for i in range(len(plan.inputs)):
                hit = next((si for si, schema in enumerate(schemas) if plan.matches(i, schema)), None)
                if hit is not None:
                    yield plan, i, hit

    def feed_device_sources(self, sources, borrow: bool = False, pane: Optional[int] = None):
        """feed_data_sources for relations that already lie in device memory: `sources` = [(columns, valid)], each as `_Plan.feed_columns`
        takes them (what csv_decode / event_source return).  Every source goes to every plan leaf whose columns it covers.  `borrow`: the
        tensors stay unchanged until clean_data_sources, and the library may read them in place.  `pane`: with an open window ring the
        sources are ONE pane (what `device_panes` cuts a batch into).  A pane's rows are copied into the ring, so here a source goes to ONE
        leaf of a plan -- the first whose columns it covers, feed_data_sources' rule, which is what lets host panes and device panes
        alternate in one ring (q5's second `bid` scan reads the first's rows either way) -- and a plan that no source matched gets the empty
        pane, as feed_data_sources(sources, pane) gives it.  Returns how many leaves were fed."""
        if self._ring and pane is None:
            raise ValueError("feed_device_sources: a window ring takes panes from the host (feed_data_sources(sources, pane))")
        if pane is not None and not self._ring:
            raise ValueError("feed_device_sources: `pane` goes with an open window ring")
        fed = 0
        if pane is None:
            for plan, i, si in list(self._device_leaf_sources(sources)):
                columns, valid = sources[si]
                plan.feed_columns(i, columns, valid, borrow)
                fed += 1
            return fed
        schemas = [_columns_schema(columns) for columns, _ in sources]
        for plan in self.plans:
            used = set()
            for i in range(len(plan.inputs)):
                hit = next((si for si, schema in enumerate(schemas) if si not in used and plan.matches(i, schema)), None)
                if hit is not None:
                    used.add(hit)
                    plan.feed_columns(i, sources[hit][0], sources[hit][1], borrow, pane)
                    fed += 1
            if not used and plan.inputs:   # nothing arrived in this pane: the ring still advances
                plan.feed_columns(0, [], None, False, pane)
        return fed

    def result_columns(self, plan: int = 0):
        """After execute_retain(): plan `plan`'s result as (columns, valid, rows), borrowed views in csv_encode's argument shape."""
        return self.plans[plan].result_columns()

    def prefetch_data_sources(self, sources, pane: int):
        """The sources of pane `pane` -- the ring's NEXT pane -- matched to the leaves as feed_data_sources matches them; what a prefetch
        takes (columns without NULLs, one leaf per plan) starts crossing PCIe now, beside the current window's execute, the
        rest is kept and fed the ordinary way by `feed_data_sources(None, pane)`."""
        if not self._ring:
            raise ValueError("prefetch_data_sources: open a window ring first")
        pre = {"pane": pane, "moving": [], "later": []}
        started = set()
        for plan, i, batches in self._leaf_sources(sources):
            if id(plan) not in started and plan.prefetch(i, batches, pane):
                started.add(id(plan))
                pre["moving"].append((plan, i))
            else:
                pre["later"].append((plan, i, batches))
        self._pre = pre

    def share_data_sources(self, donor: "ExecutionContext") -> bool:
        """Instead of feed_data_sources: every leaf reads, in place, the relation of the same name that `donor` (another function
        hosted on the same GPU context, already fed and not yet cleaned) holds on the device.  All leaves or none: False when a
        leaf finds no such relation or the donor does not keep a column it reads -- feed this context its own copy then."""
        pairs = []
        for plan in self.plans:
            for i, name in enumerate(plan.inputs):
                hit = next(((dp, di) for dp in donor.plans for di, dn in enumerate(dp.inputs) if dn == name and dn), None)
                if hit is None:
                    return False
                pairs.append((plan, i, hit[0], hit[1]))
        done = []
        for plan, i, dp, di in pairs:
            if not plan.feed_shared(i, dp, di):
                for q in done:
                    q.reset()
                return False
            done.append(plan)
        return True

    def execute_retain(self):
        """execute, with every plan's result left on the device (`_Plan.execute_retain`): [rows per plan]."""
        return [plan.execute_retain() for plan in self.plans]

    def exchange_retain(self, comm, gather_rank: int = -1, no_rows: bool = False):
        """execute_retain across the ranks of `comm` (`_Plan.exchange_retain`), plan after plan: [rows received per plan]."""
        return [plan.exchange_retain(comm, gather_rank, no_rows) for plan in self.plans]

    def feed_from(self, producers: Sequence["ExecutionContext"]):
        """feed_data_sources from stages hosted on the same GPU context: every leaf takes the first remaining producer plan whose
        retained result holds the columns it reads (matched by name and type, as compare_schema matches batches).  A leaf that
        feed_data_sources / share_data_sources already gave a base relation keeps it: a stage may read one next to its producers
        (a union of a scan and an aggregate, cut at the aggregate's repartition).  Returns how many producer plans found a leaf."""
        left = [p for ctx in producers for p in ctx.plans]
        taken = 0
        for plan in self.plans:
            for i in range(len(plan.inputs)):
                if i in plan._base_fed:
                    continue
                hit = next((p for p in left if plan.feed_from(i, p)), None)
                if hit is not None:
                    left.remove(hit)
                    taken += 1
        return taken

    def _concurrent(self) -> bool:   # every plan on its own GpuContext: their executes can be in flight together
        return len(self.plans) > 1 and len({id(p.gpu) for p in self.plans}) == len(self.plans)

    # -- context.rs:172-191: one task per plan, then join them all
    def _join_all(self, started, unwrap):
        """Joins EVERY started plan, then raises the first error: a plan whose execute is never waited for keeps `async_pending` and refuses
        every later feed / reset / execute -- the reference's `futures::join_all` also awaits every task before `?`."""
        out, first = [], None
        for plan in started:
            try:
                out.append(unwrap(plan.wait()))
            except Exception as e:   # noqa: BLE001 -- collected, re-raised below
                first = first or e
                out.append(None)
        if first is not None:
            raise first
        return out

    def _start_all(self, partitioned: bool):
        started = []
        try:
            for plan in self.plans:
                plan.execute_async(partitioned)
                started.append(plan)
        except Exception:
            for plan in started:   # what did start is joined before the error leaves
                try:
                    plan.wait()
                except Exception:   # noqa: BLE001
                    pass
            raise
        return started

    def execute(self):
        if self._concurrent():
            return self._join_all(self._start_all(False), lambda b: [b])
        return [[plan.execute()] for plan in self.plans]

    # -- context.rs:197-216: [plan][partition][batch]; a shuffling stage returns its P hash partitions
    def execute_partitioned(self):
        if self._concurrent():
            return self._join_all(self._start_all(True), lambda bs: [[b] for b in bs])
        return [[[b] for b in plan.execute_partitioned()] for plan in self.plans]

    # -- context.rs:227-254
    def clean_data_sources(self):
        for plan in self.plans:
            plan.reset()

    # -- context.rs:328-337
    def is_shuffling(self) -> bool:
        """Every plan ends in `CoalesceBatchesExec <- RepartitionExec Hash` (a RoundRobin repartition shuffles nothing)."""
        return bool(self.plans) and all(p.is_shuffling for p in self.plans)

    def schema(self, index: int):
        """Output schema of plan `index` (context.rs:222-224): taken from an execution over the current inputs."""
        return self.plans[index].execute().schema

    def close(self):
        for p in self.plans:
            p.close()
        if self._owns_gpu:
            self._gpu.close()


def explain(plan: Union[str, dict]) -> str:
    """Host-only: the operator tree of `plan` with derived schemas and the executor of every node (no GPU needed)."""
    raw = (plan if isinstance(plan, str) else json.dumps(plan)).encode()
    buf = C.create_string_buffer(1 << 16)
    rc = _ffi.load().flockgpu_plan_explain(raw, len(raw), buf, len(buf))
    text = buf.value.decode()
    if rc != 0:
        raise FlockGpuError(rc, text)
    return text


def partition_scheme() -> str:
    """How this library's shuffling stages place rows (flockgpu_plan_partition_scheme): a scheduler compares it across the
    producers of a stage before it starts them -- mixed placements split one key over two consumers."""
    return _ffi.load().flockgpu_plan_partition_scheme().decode()


def collect(ctx: ExecutionContext, streams, pane: Optional[int] = None):
    """`actor::collect` (flock-function/src/aws/actor.rs:54-79): feed -> execute -> clean.  With an open window ring `streams`
    is ONE pane and the result is the window that pane completes (hopping.rs:52-74 without the re-send)."""
    ctx.feed_data_sources(streams, pane)
    if ctx.is_shuffling():
        out = ctx.execute_partitioned()
        assert len(out) == 1
        out = out[0]
    else:
        out = ctx.execute()
    ctx.clean_data_sources()
    return out


def collect_device(ctx: ExecutionContext, sources, pane: Optional[int] = None):
    """`collect` for relations that already lie in device memory (`feed_device_sources`): feed -> execute -> clean.  With an open window
    ring `sources` is ONE pane (an entry of `device_panes`) and the result is the window that pane completes."""
    ctx.feed_device_sources(sources, pane=pane)
    if ctx.is_shuffling():
        out = ctx.execute_partitioned()
        assert len(out) == 1
        out = out[0]
    else:
        out = ctx.execute()
    ctx.clean_data_sources()
    return out


def device_panes(gpu: GpuContext, columns, valid, time_column: str, hop_ms: int, origin_ms: int = 0, max_panes: int = 4096):
    """A batch of device columns cut into the panes of a hopping window by event time (`GpuContext.pane_split` on column `time_column`):
    [(pane_id, columns_k, valid_k)] for every pane from the first present to the last, panes in between that hold no row included with zero
    rows -- each entry what `feed_device_sources([(columns_k, valid_k)], pane=pane_id)` takes.  The entries are views of the batch: tensors
    are sliced, a DeviceUtf8 is sliced with its offsets as they are (the feed rebases them).  Rows that are not in pane order are brought
    into it first, with ONE take per column and validity column (stable: arrival order is kept inside a pane)."""
    valid = dict(valid or {})
    hit = [col for name, _, col in columns if name == time_column]
    if not hit or isinstance(hit[0], DeviceUtf8):
        raise ValueError(f"device_panes: no fixed-width column {time_column!r}")
    first, bounds, rows = gpu.pane_split(hit[0], hop_ms, origin_ms, valid.get(time_column), max_panes)
    if rows is not None:
        import torch
        slot, taken = 0, []
        for name, t, col in columns:
            if isinstance(col, DeviceUtf8):
                col, slot = gpu.take_utf8(col, rows, slot), slot + 1
            elif t == "float64":
                col = gpu.take(col.view(torch.int64), rows).view(torch.float64)
            else:
                col = gpu.take(col, rows)
            taken.append((name, t, col))
        columns, valid = taken, {name: gpu.take(v, rows) for name, v in valid.items()}
    out = []
    for k in range(len(bounds) - 1):
        lo, hi = int(bounds[k]), int(bounds[k + 1])
        cols_k = [(name, t, DeviceUtf8(col.offsets[lo:hi + 1], col.data) if isinstance(col, DeviceUtf8) else col[lo:hi]) for name, t, col in columns]
        out.append((first + k, cols_k, {name: v[lo:hi] for name, v in valid.items()}))
    return out
