"""CPU reference for UnionExec (union.hpp A-U1..7), in plain Python: a table is a list of row tuples, None is NULL.

  A-U1  names come from input 0; every input has its column count and, per column, its type -- otherwise ValueError naming the input, the column
        and both types; a column is nullable when it is nullable in any input.
  A-U2  all rows of input 0 in their order, then input 1's, and so on.
  A-U3  nothing is compared: a NULL travels verbatim.
  A-U4  an empty input contributes nothing; every input empty gives no rows.
  A-U5  only the columns somebody reads are produced (`keep`); with none kept the answer is the row count alone.
  A-U6  2^31 rows or more, or 2^31 bytes or more in a Utf8 column, are refused (`check_limits`, from counts alone).
  A-U7  a relation scanned by several branches is ONE table: every branch sees all of its rows and columns (the tests feed it once).
Filters, projections and aggregates around a union are composed with plain Python by the tests."""

LIMIT = 1 << 31


def union_schema(schemas):
    """schemas: per input a list of (name, type, nullable).  The union's schema (A-U1), or ValueError."""
    if not schemas:
        raise ValueError("Union: no inputs")
    first = schemas[0]
    out = [list(f) for f in first]
    for k, sch in enumerate(schemas[1:], 1):
        if len(sch) != len(first):
            raise ValueError("Union: input %d has %d columns, input 0 has %d" % (k, len(sch), len(first)))
        for i, (name, ty, nullable) in enumerate(sch):
            if ty != first[i][1]:
                raise ValueError("Union: input %d gives %s for column %d ('%s'), input 0 gives %s" % (k, ty, i, name, first[i][1]))
            out[i][2] = out[i][2] or nullable
    return [tuple(f) for f in out]


def union_rows(inputs, keep=None):
    """inputs: lists of row tuples of one width.  Their rows one input after the other (A-U2..4); keep: the column positions produced (A-U5)."""
    rows = [r for inp in inputs for r in inp]
    if keep is None:
        return rows
    return [tuple(r[c] for c in keep) for r in rows]


def union_count(inputs):
    """A-U5: COUNT(*) over a union reads no column."""
    return sum(len(inp) for inp in inputs)


def rows_of(table, names):
    """Row tuples of a column table {name: list} over `names`."""
    return list(zip(*[table[c] for c in names])) if names else []


def union_table(tables):
    """Column tables {name: list} in (columns matched by POSITION), column table out under input 0's names."""
    names = list(tables[0])
    for k, t in enumerate(tables):
        if len(t) != len(names):
            raise ValueError("Union: input %d has %d columns, input 0 has %d" % (k, len(t), len(names)))
    return {name: [v for t in tables for v in t[list(t)[i]]] for i, name in enumerate(names)}


def check_limits(row_counts, byte_counts=()):
    """A-U6 from counts alone: raises ValueError at 2^31 rows / bytes."""
    if sum(row_counts) >= LIMIT:
        raise ValueError("Union: more than 2^31 rows")
    if sum(byte_counts) >= LIMIT:
        raise ValueError("Union: a Utf8 column exceeds 2^31 bytes")
