"""CPU reference for CrossJoinExec (cross.hpp A-X1..6), in plain Python: a table is a list of row tuples, None is NULL.

  A-X1  the output row is the left row's values followed by the right row's.
  A-X2  every (left row i, right row j) exactly once; pair (i, j) is output row i * R + j (left-major).
  A-X3  nothing is compared: a NULL travels verbatim.
  A-X4  an empty side gives no rows.
Filters, projections and aggregates above a cross join are composed with oracle/generic_ops.py by the tests."""


def cross_rows(left, right):
    """left, right: lists of row tuples; the L * R output rows in order."""
    return [l + r for l in left for r in right]


def rows_of(table, names):
    """Row tuples of a column table {name: list} over `names`."""
    return list(zip(*[table[c] for c in names])) if names else []


def cross_table(left, right):
    """Column tables {name: list} in, column table out (left columns first; the two sides' names are disjoint)."""
    ln, rn = list(left), list(right)
    rows = cross_rows(rows_of(left, ln), rows_of(right, rn))
    cols = list(zip(*rows)) if rows else [()] * (len(ln) + len(rn))
    return {name: list(cols[i]) for i, name in enumerate(ln + rn)}
