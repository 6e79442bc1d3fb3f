"""CPU reference for HashJoinExec join_type Semi / Anti (relops.hpp A-S1..5), in plain Python: tables are dicts of equally long lists, None is NULL.

  A-S1  Semi keeps the left rows for which at least one right row is equal in every key pair, Anti those for which none is.
  A-S3  a left row is kept at most once; left rows with equal keys are judged each on its own.
  A-S4  a NULL in any key column equals nothing: such a right row never matches, such a left row is dropped by Semi and kept by Anti.
  A-S5  rows come out in left input order.
Integers compare by value across widths (an Int32 column meets an Int64 one), strings bytewise."""


def semi_anti_rows(left, right, on, anti):
    """The kept row numbers of `left`, ascending.  on = [(left column, right column), ...]."""
    lcols = [left[a] for a, _ in on]
    rcols = [right[b] for _, b in on]
    n_left = len(lcols[0]) if lcols else 0
    n_right = len(rcols[0]) if rcols else 0
    present = set()
    for j in range(n_right):
        key = tuple(c[j] for c in rcols)
        if all(v is not None for v in key):
            present.add(key)
    keep = []
    for i in range(n_left):
        key = tuple(c[i] for c in lcols)
        hit = all(v is not None for v in key) and key in present
        if hit != bool(anti):
            keep.append(i)
    return keep


def semi_anti_table(left, right, on, anti):
    """The left table restricted to the kept rows (A-S2: the left input's columns, nothing of the right side)."""
    rows = semi_anti_rows(left, right, on, anti)
    return {c: [v[i] for i in rows] for c, v in left.items()}


def table_rows(t, cols):
    """Row tuples of `t` over the column names `cols`."""
    return list(zip(*[t[c] for c in cols])) if cols else []
