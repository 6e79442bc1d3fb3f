"""q5 outside the count pass: the max pass in packed 16-bit arithmetic, tiles wider than the count pass's LDS histogram, the results learnt
by polling with the clean-up queued behind the finish kernel -- against the CPU oracle, window by window.

Every case runs on a fresh GpuContext and calls at least three times (the first call lays the counters out on the host, the following
ones take the speculated path), and compares, per window: the winners (auctions, counts, offsets) with oracle.q5_hot_items, win_max()
with the numpy maximum count and win_groups() with the number of distinct keys.  The group count comes out of the packed path's dot
products and no other test pins it.

Sizes the cases lean on (flock_amd/csrc/q5.hip): two 16-bit counters share a 32-bit word, eight a 16-byte group, and pane bases are
multiples of 8 (test_gpu_q5_small_passes._layout); a window count is the packed SATURATING sum of its two panes' counts; a tile is 8192
rows from the 4-row-aligned row at or below its pane's start, "wide" when its keys span 4096 or more."""
import numpy as np
import pytest

import oracle
from test_gpu_q5_small_passes import _Case as _SmallCase, _hopping, _layout, _pane, _tumbling

pytestmark = pytest.mark.gpu

CALLS = 3
TILE = 8192


class _Case(_SmallCase):
    """test_gpu_q5_small_passes._Case + the windows' maximum and group count (numpy), computed once per row range."""

    def stats(self, lo, hi):
        key = ("stats", lo, hi)
        if key not in self._ref:
            _, cnt = np.unique(self.auction[lo:hi], return_counts=True)
            self._ref[key] = (int(cnt.max()) if len(cnt) else 0, len(cnt))
        return self._ref[key]

    def check(self, ctx, win_lo, win_hi):
        from flock_amd import WindowSchedule
        sched = WindowSchedule(self.offs, win_lo, win_hi)
        r = ctx.q5_hot_items(self.bids(), sched)
        a, n, off = r.to_host()
        mx, groups = r.win_max(), r.win_groups()
        assert off[0] == 0 and off[-1] == len(a) == len(n)
        for w in range(sched.n_windows):
            lo, hi = sched.window_rows(w)
            got = sorted(zip(a[off[w]:off[w + 1]].tolist(), n[off[w]:off[w + 1]].tolist()))
            assert got == self.ref(lo, hi), (w, lo, hi)
            assert (int(mx[w]), int(groups[w])) == self.stats(lo, hi), (w, lo, hi)


def _run(case, schedules, calls=CALLS):
    from flock_amd import GpuContext
    for win_lo, win_hi in schedules:
        ctx = GpuContext(0)
        try:
            for _ in range(calls):
                case.check(ctx, win_lo, win_hi)
        finally:
            ctx.close()


# ---- 1. window counts around the 16-bit edge with both pane counts inside it ------------------------------------------------------------
@pytest.mark.parametrize("hot", [1000, 1001], ids=["even_key", "odd_key"])
@pytest.mark.parametrize("c0,c1", [(40_000, 40_000), (32_767, 32_768), (32_767, 32_767), (65_535, 1)],
                         ids=["sum_80000", "sum_65535", "sum_65534", "sum_65536"])
def test_q5_window_sum_around_16_bits_with_both_panes_below(hot, c0, c1):
    """Panes [0, half) and [half, n), windows {0, 1} and {1} (the hopping shape): one key occurs c0 / c1 times in the two panes.  Both fit a
    16-bit counter; their sum reaches or passes 65535, where the packed add stops."""
    rng = np.random.default_rng(c0 + 3 * c1 + hot)
    panes = []
    for c in (c0, c1):
        k = np.concatenate([np.full(c, hot, np.int64), 1002 + rng.integers(0, 3000, 75_000)])
        rng.shuffle(k)
        panes.append(k)
    for k in panes:
        assert np.unique(k, return_counts=True)[1].max() <= 65_535     # no pane count overflows: the packed sum is what is exercised
    case = _Case(panes)
    assert case.stats(0, len(case.auction))[0] == c0 + c1
    _run(case, [(np.array([0, 1]), np.array([2, 2]))])


# ---- 2. winner position inside a 16-byte group of counters ----------------------------------------------------------------------------
# Three panes of ~3000 rows over 20 000 keys each, every pane 10 000 keys above the one before (every 4-row group of such a pane is
# sampled, so a pane's counters are exactly _layout(lowest key, highest key)): pane 0's keys up to ~5900 above its lowest are outside
# pane 1's counters, the others inside; pane 1's keys from ~4100 above pane 0's highest are outside pane 0's counters (role a).
_SPAN, _STEP, _ROWS, _L = 20_000, 10_000, 3_000, 1_000_000


def _placed_key(place, pos):
    lo = [_L + _STEP * p for p in range(3)]
    base = [_layout(l, l + _SPAN - 1) for l in lo]
    if place == "covered":              # pane 0, in a group pane 1 covers
        pane, near = 0, lo[0] + 15_000
    elif place == "uncovered":          # pane 0, in a group pane 1 does not cover
        pane, near = 0, lo[0] + 2_000
    else:                               # "role_a": pane 1, outside pane 0's counters
        pane, near = 1, lo[1] + 17_000
    b = base[pane][0]
    key = b + (near - b) // 8 * 8 + pos
    in0 = base[0][0] <= key < base[0][0] + base[0][1]
    in1 = base[1][0] <= key < base[1][0] + base[1][1]
    assert (in0, in1) == {"covered": (True, True), "uncovered": (True, False), "role_a": (False, True)}[place]
    return pane, key, lo


@pytest.mark.parametrize("pos", range(8))
@pytest.mark.parametrize("place", ["covered", "uncovered", "role_a"])
def test_q5_winner_at_each_position_of_a_counter_group(place, pos):
    rng = np.random.default_rng(8 * pos + len(place))
    pane, key, lo = _placed_key(place, pos)
    panes = [_pane(rng, lo[p], _SPAN, _ROWS, [(key, 200)] if p == pane else [], {key}) for p in range(3)]
    case = _Case(panes)
    assert case.ref(0, 2 * _ROWS) == [(key, 200)]          # window (0, 1): the one winner
    _run(case, [_hopping(3)])


def test_q5_tie_across_two_words_of_one_group():
    rng = np.random.default_rng(5)
    _, key, lo = _placed_key("covered", 0)
    k1, k2 = key + 1, key + 2                               # second half of word 0, first half of word 1
    panes = [_pane(rng, lo[0], _SPAN, _ROWS, [(k1, 150), (k2, 90)], {k1, k2}),
             _pane(rng, lo[1], _SPAN, _ROWS, [(k1, 50), (k2, 110)], {k1, k2}),
             _pane(rng, lo[2], _SPAN, _ROWS, [], {k1, k2})]
    case = _Case(panes)
    assert case.ref(0, 2 * _ROWS) == [(k1, 200), (k2, 200)]
    _run(case, [_hopping(3), _tumbling(3)])


# ---- 3. wide tiles among narrow ones -------------------------------------------------------------------------------------------------------
def _tiles(offs):
    """(row lo, row hi) of every tile, as build_seg_tiles cuts them."""
    out = []
    for b, e in zip(offs[:-1], offs[1:]):
        out += [(max(t, b), min(t + TILE, e)) for t in range(int(b) & ~3, int(e), TILE)]
    return out


def test_q5_wide_tiles_among_narrow_ones():
    """Three panes of 3 x 8192 + 37 rows over 300 000 keys: in each pane one full tile and the ragged last one are uniform over the whole
    span (wide: counted row by row on the pane's counters), the others sit within 600 consecutive keys (the LDS histogram)."""
    rng = np.random.default_rng(37)
    n, span = 3 * TILE + 37, 300_000
    offs = np.arange(4) * n
    tiles = _tiles(offs)
    col = np.empty(3 * n, np.int64)
    for i, (lo, hi) in enumerate(tiles):
        p, t, last = lo // n, i % 4, i % 4 == 3
        base = 5_000_000 + 40_000 * p
        if t == 1 or last:
            col[lo:hi] = rng.integers(base, base + span, hi - lo)
        else:
            col[lo:hi] = base + 70_000 * t + rng.integers(0, 600, hi - lo)
        if t == 1:
            col[lo], col[lo + 1] = base, base + span - 1
    wide = sum(int(col[lo:hi].max() - col[lo:hi].min()) >= 4096 for lo, hi in tiles)
    # two of a pane's four tiles are wide: wide MODE (the partition pass) is not entered all the same -- it takes more than 64 tiles to
    # set its hint; the next test has the wide tiles under a quarter of all tiles
    assert (wide, len(tiles)) == (6, 12) and len(tiles) <= 64
    case = _Case([col[offs[p]:offs[p + 1]] for p in range(3)])
    _run(case, [_hopping(3), _tumbling(3)])


def test_q5_wide_tiles_fewer_than_a_quarter():
    """The same, with seven narrow tiles per wide one: under a quarter of the tiles are wide, as in a stream that stays on the fast kernel."""
    rng = np.random.default_rng(38)
    n, span = 8 * TILE + 37, 300_000
    offs = np.arange(4) * n
    tiles = _tiles(offs)
    col = np.empty(3 * n, np.int64)
    for lo, hi in tiles:
        p, t = lo // n, (lo - (int(offs[lo // n]) & ~3)) // TILE
        base = -150_000 + 40_000 * p                             # (keys across 0)
        if t in (1, 8):                                          # one full tile and the ragged last one
            col[lo:hi] = rng.integers(base, base + span, hi - lo)
        else:
            col[lo:hi] = base + 30_000 * t + rng.integers(0, 600, hi - lo)
        if t == 1:
            col[lo], col[lo + 1] = base, base + span - 1
    wide = sum(int(col[lo:hi].max() - col[lo:hi].min()) >= 4096 for lo, hi in tiles)
    assert 0 < wide * 4 < len(tiles)
    case = _Case([col[offs[p]:offs[p + 1]] for p in range(3)])
    _run(case, [_hopping(3), _tumbling(3)])


def test_q5_wide_tiles_without_direct_counters():
    """Keys uniform over all of int32: no pane gets a counter range, every tile is wide and goes through the LDS hash to the windows' tables."""
    rng = np.random.default_rng(39)
    col = rng.integers(-2**31, 2**31 - 1, 4 * TILE).astype(np.int64)
    col[:40] = col[40]                                           # one winner in pane 0 ...
    col[3 * TILE:3 * TILE + 25] = col[40]                        # ... found again in pane 3
    case = _Case([col[p * TILE:(p + 1) * TILE] for p in range(4)])
    _run(case, [_hopping(4), _tumbling(4)])


# ---- 4. retries with the clean-up queued before the results are known -------------------------------------------------------------------
def test_q5_declined_speculation_between_speculated_calls():
    """Stream A three times, stream B (pane ranges ten times wider: the counters A sized do not hold them, the device layout declines) once,
    A twice more -- on ONE context.  The declined attempt has cleaned up for nothing and its repeat must not trust that."""
    from flock_amd import GpuContext
    rng = np.random.default_rng(4)
    a = _Case([_pane(rng, 10_000 + 500 * p, 3_000, 20_000, [(10_100 + 500 * p, 300)]) for p in range(6)])
    b = _Case([_pane(rng, 8_000 + 5_000 * p, 30_000, 20_000, [(9_000 + 5_000 * p, 90)]) for p in range(6)])
    lo, hi = _hopping(6)
    ctx = GpuContext(0)
    try:
        for case in (a, a, a, b, a, a):
            case.check(ctx, lo, hi)
    finally:
        ctx.close()


def test_q5_many_ties_redo_then_an_ordinary_call():
    """70 000 distinct keys in one window: every one of them wins, more than the winner buffer and the finish kernel hold, so the attempt is
    redone with a larger buffer and the winners are ordered on the device.  An ordinary call follows on the same context."""
    from flock_amd import GpuContext
    rng = np.random.default_rng(7)
    ties = _Case([rng.permutation(np.arange(0, 35_000)), rng.permutation(np.arange(35_000, 70_000)), np.array([1, 1, 2])])
    assert len(ties.ref(0, 70_000)) == 70_000
    plain = _Case([_pane(rng, 10_000 + 500 * p, 3_000, 20_000, [(10_100 + 500 * p, 300)]) for p in range(3)])
    lo, hi = _hopping(3)
    ctx = GpuContext(0)
    try:
        for case in (ties, ties, ties, plain, plain):
            case.check(ctx, lo, hi)
    finally:
        ctx.close()
