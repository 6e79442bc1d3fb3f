"""q5's small passes (pane range estimate, max / select over windows of one or two panes, the tile min / max of the count pass)
against the CPU oracle, window by window, on hand-made columns that steer those kernels' loop shapes and edges.

Every case runs on a fresh GpuContext and calls at least three times: the first call lays the counters out on the host, the
following ones take the speculated path (device layout, 16-bit counters, pane-walking max / select), which is what the headline runs.

Sizes the cases lean on (flock_amd/csrc/q5.hip): a pane's counter range is [lo - m, hi + m] of its SAMPLED keys with m = max(span / 16, 4096),
cut to multiples of 8; the range kernel samples 2048 aligned 4-row groups per pane (every group of a pane of up to 8192 rows, every
stride-th = groups // 2048-th beyond); a lane of the max / select passes takes the 16-byte counter groups i, i + stride, ... of its pane;
the count pass reduces a tile's minimum and maximum over the wave with DPP row shifts / broadcasts (scan.hpp wave_min_i32 / wave_max_i32)."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

CALLS = 3


def _dev(a):
    from devmem import dev
    return dev(a)


def _layout(lo, hi):
    """(base, range) of a pane whose sampled keys span [lo, hi]: q5_pane_layout."""
    span = hi - lo
    margin = max(span // 16, 4096)
    base = (lo - margin) & ~7
    return base, ((hi + margin + 1 - base) + 7) & ~7


def _hopping(n_panes):
    lo = np.arange(n_panes - 1)
    return lo, lo + 2


def _tumbling(n_panes):
    lo = np.arange(n_panes)
    return lo, lo + 1


class _Case:
    """A column cut into panes + the oracle's answer per (lo, hi) row range, computed once and shared by all calls and schedules."""

    def __init__(self, panes):
        self.auction = np.ascontiguousarray(np.concatenate([np.asarray(p, np.int64) for p in panes]).astype(np.int32))
        self.offs = np.concatenate([[0], np.cumsum([len(p) for p in panes])]).astype(np.int64)
        self.n_panes = len(panes)
        self._ref = {}
        self._dev = None

    def ref(self, lo, hi):
        if (lo, hi) not in self._ref:
            a, n = oracle.q5_hot_items(self.auction[lo:hi])
            self._ref[(lo, hi)] = sorted(zip(a.tolist(), n.tolist()))
        return self._ref[(lo, hi)]

    def bids(self):
        from flock_amd import Bids
        if self._dev is None:
            self._dev = _dev(self.auction if len(self.auction) else np.zeros(4, np.int32))
        return Bids(auction=self._dev, rows=len(self.auction))

    def check(self, ctx, win_lo, win_hi):
        from flock_amd import WindowSchedule
        sched = WindowSchedule(self.offs, win_lo, win_hi)
        a, n, off = ctx.q5_hot_items(self.bids(), sched).to_host()
        for w in range(sched.n_windows):
            lo, hi = sched.window_rows(w)
            got = sorted(zip(a[off[w]:off[w + 1]].tolist(), n[off[w]:off[w + 1]].tolist()))
            assert got == self.ref(lo, hi), (w, lo, hi)


def _run(case, schedules, calls=CALLS):
    from flock_amd import GpuContext
    for win_lo, win_hi in schedules:
        ctx = GpuContext(0)
        try:
            for _ in range(calls):
                case.check(ctx, win_lo, win_hi)
        finally:
            ctx.close()


def _pane(rng, lo, span, rows, hot=(), avoid=()):
    """`rows` keys drawn from [lo, lo + span), both ends present; hot = ((key, count), ...) written over the draw.  Keys in `avoid` occur
    only as often as `hot` says (their drawn occurrences become `lo`), so that ties stay ties."""
    k = rng.integers(lo, lo + span, rows).astype(np.int64)
    if span > 1:
        k[np.isin(k, np.asarray(list(avoid), np.int64))] = lo
    k[0], k[1] = lo, lo + span - 1
    at = 2
    for key, cnt in hot:
        k[at:at + cnt] = key
        at += cnt
    assert at <= rows
    rng.shuffle(k)
    return k


# ---- loop shape of max / select ----------------------------------------------------------------------------------------------------
# Per-pane key spans 1 / 5 000 / 37 000 / 300 000 over ~3 000 rows: 1 026 / 1 651 / 5 651 / 42 188 groups of 8 counters per pane, i.e.
# 1, 2-3, 4-5 and 9+ groups per lane (trips of the pane walk's loop; some lanes make one trip fewer than their neighbours).
@pytest.mark.parametrize("span", [1, 5_000, 37_000, 300_000])
def test_q5_pane_walk_loop_shapes(span):
    rng = np.random.default_rng(span)
    rows, L = 3_000, 1_000_000
    half, far = span // 2, 10 * span + 200_000
    mid, X, Z = L + span // 3, L + span - 1, L + min(10, span - 1)
    A, B = L + half + span // 4, L + half + span - 1
    # winners spread over a lane's first, middle and last trips, whatever the grid: 4096 * r + 17 groups into the pane's counters
    walk = [(min(span - 1, (4096 * r + 17) * 8), 40 + r) for r in range(8)]
    keep = {mid, X, Z, A, B}
    panes = [
        _pane(rng, L, span, rows, [(L, 40), (mid, 30)], keep),                 # 0: `mid` wins window (0, 1) only as the sum 30 + 30
        _pane(rng, L, span, rows, [(X, 40), (mid, 30), (Z, 45)], keep),        # 1: identical range; alone: Z
        _pane(rng, L + half, span, rows, [(A, 35), (X, 5)], keep),             # 2: partly overlapping; window (1, 2): X in the overlap (40 + 5) ties with Z outside it
        _pane(rng, L + half, span, rows, [(B, 45), (A, 10)], keep),            # 3: identical to 2; window (2, 3): A (35 + 10) ties with B
        np.zeros(0, np.int64),                                                 # 4: empty neighbour of 3 and 5
        _pane(rng, L + far, span, rows, [(L + far + o, c) for o, c in walk[:4]]),          # 5: disjoint from 3 and 6
        _pane(rng, L + 2 * far, span, rows, [(L + 2 * far + o, c) for o, c in walk[4:]]),  # 6
        _pane(rng, L + 2 * far, span, rows, [(L + 2 * far + o, 3) for o, c in walk[4:]]),  # 7: identical to 6: its counts add to 6's
        _pane(rng, L - far, span, rows, [(L - far + span // 2, 50)]),          # 8: below everything
    ]
    case = _Case(panes)
    n = case.n_panes
    lo, hi = _hopping(n)
    # hopping without the window (7, 8) and with a pane (8) that belongs to no window
    _run(case, [(lo, hi), _tumbling(n), (lo[:-1], hi[:-1])])


def test_q5_winner_in_first_and_last_counter_group_and_straggler_tables():
    """Panes of 40 000 rows (sampling stride 4 groups: rows 8..11 mod 16 of a 16-aligned pane are never sampled).  Keys written only there
    are outside the sampled [lo, hi]: within the margin they land in the FIRST / LAST 16-byte group of the pane's counters; 1e7 away they
    go to the windows' straggler tables -- often enough to win."""
    rng = np.random.default_rng(11)
    rows, span = 40_000, 37_000
    los = [2_000_000, 2_000_000 + span // 2, 2_000_000 + span // 2, 5_000_000, 5_000_000]
    unsampled = np.flatnonzero((np.arange(rows) // 4) % 4 == 2)
    panes = []
    for p, lo in enumerate(los):
        k = rng.integers(lo, lo + span, rows).astype(np.int64)
        k[0], k[1] = lo, lo + span - 1          # (group 0: sampled)
        base, rng_len = _layout(lo, lo + span - 1)
        where = rng.permutation(unsampled)
        if p == 0:
            k[where[:60]] = base + 3                          # first group of the pane's counters
        elif p == 1:
            k[where[:60]] = base + rng_len - 2                # last group
        elif p == 2:
            k[where[:30]] = base + 1                          # first group, and in pane 1's range too: 30 + 30 below
            panes[1][where[100:130]] = base + 1
        elif p == 3:
            k[where[:70]] = lo + 10_000_000                   # straggler tables of windows (2, 3) and (3, 4)
        else:
            k[where[:20]] = lo + 10_000_000                   # adds to pane 3's outlier in window (3, 4)
            k[where[20:50]] = lo - 10_000_000
        panes.append(k)
    case = _Case(panes)
    _run(case, [_hopping(5), _tumbling(5)])


def test_q5_alternating_inputs_on_one_context():
    """Two inputs in turn on ONE context: the counter capacity, the slow-tile count and the layout the previous call left behind are wrong
    for the next one (narrow dense keys <-> wide keys with outliers and more counters)."""
    from flock_amd import GpuContext
    rng = np.random.default_rng(3)
    a = _Case([_pane(rng, 10_000 + 500 * p, 3_000, 20_000, [(10_100 + 500 * p, 300)]) for p in range(6)])
    b_panes = []
    for p in range(6):
        k = _pane(rng, -400_000 + 90_000 * p, 250_000, 20_000, [(-399_000 + 90_000 * p, 90)])
        k[np.flatnonzero((np.arange(20_000) // 4) % 2 == 1)[:40]] = 30_000_000 + p    # (sampling stride 2: odd groups are not sampled)
        b_panes.append(k)
    b = _Case(b_panes)
    lo, hi = _hopping(6)
    ctx = GpuContext(0)
    try:
        for case in (a, a, b, a, b, b, a):
            case.check(ctx, lo, hi)
    finally:
        ctx.close()


# ---- range kernel edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [
    (1001, 1002, 1003, 1001),          # panes that start at rows 1, 3, 2 mod 4
    (1, 2, 3, 3000, 2, 1),             # panes of 1-3 rows, at both ends
    (8192, 8193, 8192, 8191),          # exactly 2048 * 4 rows (every group sampled, stride 1), one more, one fewer
    (16384, 16385, 4099),              # sampling stride exactly 2, and one row more
], ids=["unaligned_starts", "tiny_panes", "8192_8193", "stride2"])
def test_q5_range_kernel_pane_edges(lens):
    rng = np.random.default_rng(sum(lens))
    panes = []
    for p, n in enumerate(lens):
        lo = 50_000 + 1_500 * p
        k = rng.integers(lo, lo + 2_000, n).astype(np.int64)
        k[0] = lo - 300 * (p % 2)                # the pane's extreme keys in its first and last row
        k[-1] = lo + 2_000 + 700 * (p % 3)
        panes.append(k)
    case = _Case(panes)
    n = len(lens)
    _run(case, [_hopping(n), _tumbling(n)])


@pytest.mark.parametrize("tail", [1, 2, 3])
def test_q5_column_length_not_a_multiple_of_4(tail):
    """The column's last 16-byte group is incomplete; the last pane's extreme key (far outside everything sampled) sits only in those rows."""
    rng = np.random.default_rng(tail)
    panes = [_pane(rng, 7_000, 1_000, 2_000) for _ in range(3)]
    last = rng.integers(7_000, 8_000, 2_000 + tail).astype(np.int64)
    last[-tail:] = 7_000 + 2_000_000
    last[:40] = 7_321
    panes.append(last)
    case = _Case(panes)
    assert len(case.auction) % 4 == tail
    _run(case, [_hopping(4), _tumbling(4)])


def test_q5_column_shorter_than_one_group():
    case = _Case([np.array([5]), np.array([5, 9])])
    _run(case, [_hopping(2), _tumbling(2)])


# ---- tile min / max of the count pass ---------------------------------------------------------------------------------------------------
def test_q5_tile_min_max_reduction_lanes():
    """8192-row tiles (lane l of wave v holds rows 1024 * it + 256 * v + 4 * l + j of the tile, it < 8, j < 4): the tile's minimum only in
    lane 63 of the last wave, its maximum only in lane 0 of the first; keys below and across 0 with a span under the 4096-bin histogram;
    a ragged tile.  The histogram is indexed from the tile minimum and flushed up to the tile maximum, so a lane the reduction drops loses
    the bins of its keys -- and those keys fill all 32 rows of their lane, which makes them the windows' winners."""
    rng = np.random.default_rng(21)
    T = 8192

    def rows_of(thread):
        return (np.arange(8)[:, None] * 1024 + thread * 4 + np.arange(4)[None, :]).ravel()

    t0 = rng.integers(100, 3_000, T).astype(np.int64)
    t0[rows_of(255)] = 1             # lane 63 of wave 3
    t0[rows_of(0)] = 4_050           # lane 0 of wave 0
    t1 = rng.integers(-1_900, 1_900, T).astype(np.int64)
    t1[rows_of(255)] = -2_047
    t1[rows_of(0)] = 2_047
    t2 = rng.integers(-9_000, -6_000, T).astype(np.int64)
    t2[rows_of(63)] = -9_500         # lane 63 of wave 0
    t2[rows_of(192)] = -5_600        # lane 0 of wave 3
    ragged = rng.integers(-50, 50, T + 1_234).astype(np.int64)
    ragged[T + 1_234 - 40:] = -3_000    # the ragged tile's only low keys, in its last rows
    ragged[T:T + 40] = 1_000
    case = _Case([t0, t1, t2, ragged, rng.integers(-50, 50, 777).astype(np.int64)])
    for p, keys in enumerate(({1, 4_050}, {-2_047, 2_047}, {-9_500, -5_600})):
        assert {k for k, _ in case.ref(p * T, (p + 1) * T)} == keys       # (the extreme keys ARE what the oracle reports for those panes)
    _run(case, [_hopping(5), _tumbling(5)])
