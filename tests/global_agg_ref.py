"""Ungrouped aggregates (HashAggregateExec without GROUP BY): the reference is oracle/generic_ops.py hash_aggregate_exec with group_by=[], unchanged.
This module only carries columns to it and back: a column is (values ndarray, valid bool ndarray); the oracle takes Python lists with None."""
import numpy as np

from oracle.generic_ops import hash_aggregate_exec

FNS = ("count", "sum", "min", "max", "avg")


def as_lists(cols):
    """{name: (values, valid)} -> the oracle's table (NULL = None; numpy scalars become Python ints / floats, so sums do not wrap)"""
    out = {}
    for name, (v, ok) in cols.items():
        vals = v.tolist()
        out[name] = [x if o else None for x, o in zip(vals, ok.tolist())]
    return out


def agg_name(fn, arg):
    return "%s(%s)" % (fn.upper(), arg or "UInt8(1)")


def reference_row(cols, aggs):
    """aggs = [(fn, column or None)] -> the ONE row the node returns, as a list in aggregate order (None = NULL)"""
    t = hash_aggregate_exec(as_lists(cols), [], [("a%d" % k, fn, arg) for k, (fn, arg) in enumerate(aggs)])
    row = [t["a%d" % k] for k in range(len(aggs))]
    assert all(len(c) == 1 for c in row), "an ungrouped aggregate returns exactly one row"
    return [c[0] for c in row]


def partial_state(cols, aggs):
    """The Partial node's state row: COUNT -> [count], SUM / MIN / MAX -> [value], AVG -> [count UInt64, sum Float64]"""
    out = []
    for fn, arg in aggs:
        if fn == "avg":
            c, = reference_row(cols, [("count", arg)])
            s, = reference_row(cols, [("sum", arg)])
            out += [c, float(s) if s is not None else 0.0]
        else:
            out += reference_row(cols, [(fn, arg)])
    return out


def reference_is_exact(cols, aggs, result_range):
    """The conditions under which the oracle's arithmetic is exact: every SUM inside its result type, every prefix of an AVG's Float64 sum equal
    to the exact integer sum (below 2^53 in magnitude, or -- UInt64 values at and above 2^63 -- multiples of a power of two that keep 53 bits),
    Float64 columns without NaN and without both zeros."""
    for fn, arg in aggs:
        if arg is None:
            continue
        v, ok = cols[arg]
        if v.dtype == np.float64:
            x = v[ok]
            if np.isnan(x).any() or (np.any(np.signbit(x) & (x == 0)) and np.any(~np.signbit(x) & (x == 0))):
                return False
            continue
        vals = [int(x) for x in v[ok].tolist()]
        if fn == "sum":
            lo, hi = result_range[arg]
            if vals and not (lo <= sum(vals) <= hi):
                return False
        if fn == "avg":
            exact, f = 0, 0.0
            for x in vals:
                exact += x
                f += float(x)
                if int(f) != exact:
                    return False
    return True
