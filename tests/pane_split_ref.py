"""A row-at-a-time reference of flockgpu_pane_split (csrc/panes.hpp A-PN1..11): Python integers, floor division, stable grouping."""

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
MAX_CAPACITY = 65536


class Refused(Exception):
    """code: "INVALID" | "UNSUPPORTED"; names: the numbers the message must name"""

    def __init__(self, code, names=()):
        super().__init__(code, names)
        self.code, self.names = code, tuple(names)


def pane_of(t, origin, hop):
    return (int(t) - int(origin)) // int(hop)       # Python's // rounds towards minus infinity; its integers do not overflow


def threshold(p, origin, hop):
    return int(origin) + int(p) * int(hop)


def pane_split(times, hop, origin=0, valid=None, capacity=4096):
    """-> (first_pane, bounds, rows): rows is None when the pane ids never decrease along the rows, else the stable permutation."""
    times = [int(t) for t in times]
    n = len(times)
    if hop <= 0 or not 1 <= capacity <= MAX_CAPACITY or not 0 <= n < (1 << 31):
        raise Refused("INVALID")
    if n == 0:
        return 0, [0], None
    if valid is not None:
        for i in range(n):
            if not valid[i]:
                raise Refused("INVALID", (i,))
    ids = []
    for t in times:
        p = pane_of(t, origin, hop)
        if not INT64_MIN <= p <= INT64_MAX:
            raise Refused("INVALID")
        ids.append(p)
    first, last = min(ids), max(ids)
    if last - first + 1 > capacity:
        raise Refused("UNSUPPORTED", (first, last, capacity))
    ordered = True
    for i in range(1, n):
        if ids[i] < ids[i - 1]:
            ordered = False
            break
    groups = [[] for _ in range(last - first + 1)]
    for i in range(n):                               # stable: a pane's rows in arrival order
        groups[ids[i] - first].append(i)
    bounds = [0]
    for g in groups:
        bounds.append(bounds[-1] + len(g))
    rows = None if ordered else [i for g in groups for i in g]
    return first, bounds, rows
