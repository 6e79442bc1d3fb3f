"""GROUP BY with up to sixteen accumulators per node (flock_amd/csrc/groupwide.hpp): the reference is a plain-Python restatement over dicts of lists with
None = NULL, held to pyarrow's Table.group_by in tests/test_plan_wide_group_by.py.  Group keys are tuples (a NULL key column is None: NULL keys form one
group); groups come out in order of first appearance.  The rules, one function per aggregate:
  COUNT(*) the rows; COUNT(col) the rows whose col is not NULL -- 0, never NULL;
  SUM of integers wraps in 64 bits (two's complement for Int32 / Int64 / Timestamp, modulo 2^64 for UInt64); no valid value -> NULL;
  MIN / MAX by value (Float64: -0.0 below +0.0, no NaN); no valid value -> NULL;
  AVG = double(the wrapped integer sum, read as signed) / double(count); no valid value -> NULL."""
import math

M64 = 1 << 64


def agg_name(i, fn, arg):
    """the name of entry i of an aggregate list: the same function may stand over the same column more than once"""
    return "a%d:%s(%s)" % (i, fn.upper(), arg or "UInt8(1)")


def _live(vals):
    return [v for v in vals if v is not None]


def count(vals, n_rows):
    return n_rows if vals is None else len(_live(vals))


def wrapped_sum(vals, unsigned=False):
    live = _live(vals)
    if not live:
        return None
    s = sum(live) % M64
    return s if unsigned or s < M64 // 2 else s - M64


def _order(v):
    return (v, math.copysign(1.0, v)) if isinstance(v, float) else (v, 0)


def minimum(vals):
    live = _live(vals)
    return min(live, key=_order) if live else None


def maximum(vals):
    live = _live(vals)
    return max(live, key=_order) if live else None


def avg(vals):
    live = _live(vals)
    return float(wrapped_sum(live)) / float(len(live)) if live else None


def finish(fn, vals, n_rows, unsigned=False):
    if fn == "count":
        return count(vals, n_rows)
    if fn == "sum":
        return wrapped_sum(vals, unsigned)
    return {"min": minimum, "max": maximum, "avg": avg}[fn](vals)


def aggregate(table, keys, aggs, types=None):
    """table: {column: [values]}; keys: key column names; aggs: [(fn, column or None)]; types: {column: type name} ("UInt64" sums wrap unsigned).
    -> rows (key values..., aggregate values...) in order of first appearance."""
    n = len(next(iter(table.values()))) if table else 0
    groups = {}
    for i in range(n):
        groups.setdefault(tuple(table[k][i] for k in keys), []).append(i)
    out = []
    for key, rows in groups.items():
        row = list(key)
        for fn, arg in aggs:
            row.append(finish(fn, None if arg is None else [table[arg][i] for i in rows], len(rows), bool(types) and arg is not None and types.get(arg) == "UInt64"))
        out.append(tuple(row))
    return out


def sort_rows(rows, n_keys):
    """rows sorted by key, a NULL key first (callers compare multisets: the order of the groups is the node's business)"""
    return sorted(rows, key=lambda r: tuple((0, 0) if v is None else (1, v) for v in r[:n_keys]))


def same_rows(got, want):
    """equal, and equal in the SIGN of every Float64 zero too (-0.0 == 0.0 in Python)"""
    def bits(rows):
        return [tuple((v, math.copysign(1.0, v)) if isinstance(v, float) else v for v in r) for r in rows]
    return bits(got) == bits(want)
