"""COUNT(DISTINCT x) (flock_amd/csrc/distinct.hpp A-D1..A-D7): the reference is a plain-Python restatement -- a set of values per group -- held to pyarrow's
count_distinct in tests/test_plan_count_distinct.py.  Columns are Python lists with None = NULL; group keys are tuples (a NULL key column is None: NULL keys
form one group).  The ordinary aggregates that may stand beside a distinct count (COUNT(*), COUNT(col), SUM, MIN, MAX, AVG) are restated the same way."""


def dc_name(arg):
    return "COUNT(DISTINCT %s)" % arg


def agg_name(fn, arg):
    return dc_name(arg) if fn == "dc" else "%s(%s)" % (fn.upper(), arg or "UInt8(1)")


def _finish(fn, vals, n_rows):
    """one aggregate over the group's argument values (NULLs still in)"""
    if fn == "count" and vals is None:
        return n_rows
    live = [v for v in vals if v is not None]
    if fn == "dc":
        return len(set(live))                     # A-D1: distinct non-NULL values; no valid value -> 0, never NULL
    if fn == "count":
        return len(live)
    if not live:
        return None
    if fn == "sum":
        return sum(live)
    if fn == "min":
        return min(live)
    if fn == "max":
        return max(live)
    if fn == "avg":                               # one IEEE division of (double) sum by (double) count
        return float(sum(live)) / float(len(live))
    raise ValueError(fn)


def aggregate(table, keys, aggs):
    """table: {column: [values]}; keys: key column names ([] = no GROUP BY: exactly one row, over no rows too); aggs: [(fn, column or None)], fn "dc" =
    COUNT(DISTINCT column).  -> rows (key values..., aggregate values...) in order of first appearance."""
    n = len(next(iter(table.values()))) if table else 0
    groups = {}
    if not keys:
        groups[()] = list(range(n))
    for i in range(n if keys else 0):
        groups.setdefault(tuple(table[k][i] for k in keys), []).append(i)
    out = []
    for key, rows in groups.items():
        row = list(key)
        for fn, arg in aggs:
            row.append(_finish(fn, None if arg is None else [table[arg][i] for i in rows], len(rows)))
        out.append(tuple(row))
    return out


def sort_rows(rows, n_keys):
    """rows sorted by key, a NULL key first (the order of the output groups is unspecified, A-D6)"""
    return sorted(rows, key=lambda r: tuple((0, 0) if v is None else (1, v) for v in r[:n_keys]))
