"""Helpers of tests/test_plan_device_feed.py: one table of plan_corpus.make_table's shape as host record batches and as device columns, the plans the
tests run (plan_corpus' builders), and the row normalisation of tests/test_plan_differential.py."""
import random
import struct

import numpy as np
import pyarrow as pa

import null_poison as npz
import plan_corpus as pc
import plan_interp as pi

FLAG_TILE = 8192            # scan.hpp kFlagTile
_PA = {"Int32": pa.int32(), "Int64": pa.int64(), "UInt64": pa.uint64(), "Float64": pa.float64(), "Utf8": pa.string()}
_DEV = {"Int32": ("int32", np.int32), "Int64": ("int64", np.int64), "UInt64": ("uint64", np.uint64), "Float64": ("float64", np.float64)}


def arrow_type(t):
    return pa.timestamp("ms") if isinstance(t, dict) else _PA[t]


def norm(rows):
    """floats by their bits, text as bytes"""
    def one(v):
        if isinstance(v, float):
            return ("f", struct.unpack("<q", struct.pack("<d", v))[0])
        return v.encode() if isinstance(v, str) else v
    return [tuple(one(v) for v in r) for r in rows]


def multiset(rows):
    return sorted(rows, key=lambda r: tuple((0, 0) if v is None else (1, repr(type(v)), v) for v in r))


def batch_rows(batches):
    rows = []
    for rb in batches:
        cols = [(c.cast(pa.int64()) if pa.types.is_timestamp(c.type) else c).to_pylist() for c in rb.columns]
        rows += list(zip(*cols)) if cols else []
    return rows


def host_batch(fields, table, lo=0, hi=None, poison=None, leaf=0):
    """poison: None, or (pool, key) -- the NULL slots hold tests/null_poison.py's values for leaf `leaf` of that key"""
    arrs = []
    for f in fields:
        if poison is not None:
            arrs.append(npz.poisoned_column(poison[0], poison[1], leaf, f["name"], table[f["name"]], f["data_type"], lo, hi))
            continue
        ty, vals = arrow_type(f["data_type"]), table[f["name"]][lo:hi]
        arrs.append(pa.array(vals, pa.int64()).cast(ty) if pa.types.is_timestamp(ty) else pa.array(vals, ty))
    return pa.record_batch(arrs, names=[f["name"] for f in fields])


def device_source(fields, table, lo=0, hi=None, device="cuda:0", validity="nulls", shift=0, null_slot=0, poison=None, leaf=0):
    """Rows [lo, hi) of `table` as (columns, valid) for feed_columns.  validity: "nulls" -- validity bytes for the columns that hold a NULL in these
    rows; "always" -- for every column, all 1 where there is none.  shift: every tensor is the [shift:] slice of a larger one (values, validity and
    offsets alike: element-aligned, not 16-byte aligned) and a Utf8 column's offsets start at 3 instead of 0.  NULL slots hold `null_slot` / '' -- or, poison = (pool, key), what tests/null_poison.py puts under the NULLs of leaf
    `leaf` of that key: values of the pool, and BYTES under the NULL rows of a Utf8 column (a row's poison does not depend on lo and hi)."""
    import torch
    from flock_amd.engine import DeviceUtf8

    def dev(arr):
        whole = np.concatenate([np.full(shift, 0x55, arr.dtype), arr]) if shift else arr
        return torch.from_numpy(np.ascontiguousarray(whole)).to(device)[shift:]

    columns, valid = [], {}
    for f in fields:
        name, t = f["name"], f["data_type"]
        vals = table[name][lo:hi]
        under = npz.slots(poison[0], *poison[1], leaf, name, table[name], t)[lo:hi] if poison is not None else None
        ok = np.array([v is not None for v in vals], np.uint8)
        if validity == "always" or not ok.all():
            valid[name] = dev(ok)
        if t == "Utf8":
            raw = under if under is not None else [b"" if v is None else v.encode() for v in vals]
            junk = b"\x01\x02\x03" if shift else b""
            off = np.zeros(len(raw) + 1, np.int32)
            off[1:] = np.cumsum([len(b) for b in raw], dtype=np.int64)
            data = np.frombuffer(junk + b"".join(raw) + b"\0" * 16, np.uint8).copy()
            columns.append((name, "utf8", DeviceUtf8(dev(off + len(junk)), torch.from_numpy(data).to(device))))
            continue
        kind, dtype = ("timestamp_ms", np.int64) if isinstance(t, dict) else _DEV[t]
        arr = npz.numeric_slots(under, t) if under is not None else np.array([null_slot if v is None else v for v in vals], dtype=dtype)
        if dtype is np.uint64:
            arr = arr.view(np.int64)
        columns.append((name, kind, dev(arr)))
    return columns, valid


# ------------------------------------------------------------------ tables and plans
def table(prefix, n, seed, **kw):
    r, rnd = np.random.default_rng(seed * 7919 + n), random.Random(seed * 7919 + n)
    kw.setdefault("style", "dense")
    kw.setdefault("card", 50)
    kw.setdefault("groups", 5)
    kw.setdefault("nulls", {"u": 0.02, "t": 0.02, "f": 0.02, "s": 0.3, "s2": 0.02, "v": 0.02, "i": 0.02})
    kw.setdefault("key_nulls", 0.15)
    return pc.make_table(prefix, n, r, rnd, **kw)


def build_side(n=300, seed=5):
    """300 rows with unique keys -7, -4, ..: a third of the dense probe keys -16 .. 33 find one partner"""
    return table("b", n, seed, style="unique", key_nulls=0.02)


# filter_plain: filter_project's plan over a table WITHOUT a NULL in the columns the feed may drop rows by (a_k, a_l, a_g): nothing is left out, every
# column -- Utf8 and validity included -- takes the plain append
KINDS = ("filter_project", "filter_plain", "group_by", "join_inner", "join_semi", "global_agg", "sort_limit")
PLAIN = dict(key_nulls=0.0)


def plan_of(kind):
    """-> (plan, the prefixes of its tables in leaf order, ordered)"""
    a, b = pc.scan(pc.table_cols("a")), pc.scan(pc.table_cols("b"))
    if kind in ("filter_project", "filter_plain"):
        node = pc.keep(pc.filt(a, pc.binop(a.c("a_g"), "Lt", pc.lit("Int32", 3))), ["a_id", "a_k", "a_l", "a_u", "a_t", "a_f", "a_s", "a_s2", "a_i"])
        return node.plan, ["a"], False
    if kind == "group_by":
        return pc.aggregate(a, ["a_g"], [("count", None), ("sum", "a_v"), ("min", "a_i"), ("max", "a_l")]).plan, ["a"], False
    if kind == "join_inner":
        node = pc.join("Inner", pc.keep(b, ["b_k", "b_id", "b_u", "b_s"]), pc.keep(a, ["a_k", "a_id", "a_s2", "a_f"]), [("b_k", "a_k")])
        return node.plan, ["b", "a"], False
    if kind == "join_semi":
        node = pc.join("Semi", pc.keep(a, ["a_k", "a_id", "a_s2", "a_v"]), pc.keep(b, ["b_k", "b_s2"]), [("a_k", "b_k")])
        return node.plan, ["a", "b"], False
    if kind == "global_agg":
        return pc.aggregate(a, [], [("count", None), ("max", "a_u"), ("sum", "a_v"), ("min", "a_f"), ("count", "a_f")]).plan, ["a"], False
    assert kind == "sort_limit", kind
    node = pc.limit(pc.sort(pc.keep(a, ["a_t", "a_id", "a_v", "a_s"]), [("a_t", False, False), ("a_id", False, False)]), 50)
    return node.plan, ["a"], True


class Run:
    """One plan on one context: feeds by table (leaf order of plan_interp.leaf_schemas), host or device, then the rows."""

    def __init__(self, gpu, plan, generic_only=False):
        from flock_amd.runtime import ExecutionContext
        self.gpu, self.plan = gpu, plan
        self.ctx = ExecutionContext([plan], gpu=gpu, generic_only=generic_only)
        self.p = self.ctx.plans[0]
        self.fields = pi.leaf_schemas(plan)
        self.leaf, used = [], set()
        for fields in self.fields:
            schema = pa.schema([(f["name"], arrow_type(f["data_type"])) for f in fields])
            i = next(i for i in range(len(self.p.inputs)) if i not in used and self.p.matches(i, schema))
            used.add(i)
            self.leaf.append(i)

    def host(self, t, table, lo=0, hi=None, poison=None):
        self.p.feed(self.leaf[t], [host_batch(self.fields[t], table, lo, hi, poison=poison, leaf=t)])

    def device(self, t, table, lo=0, hi=None, borrow=False, **kw):
        columns, valid = device_source(self.fields[t], table, lo, hi, device=f"cuda:{self.gpu.device}", leaf=t, **kw)
        self.p.feed_columns(self.leaf[t], columns, valid, borrow=borrow)
        return columns, valid

    def rows(self, ordered=False):
        got = norm(batch_rows([self.p.execute()]))
        return got if ordered else multiset(got)

    def close(self):
        self.ctx.close()
