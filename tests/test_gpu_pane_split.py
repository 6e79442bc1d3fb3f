"""flockgpu_pane_split on the device against the row-at-a-time reference (tests/pane_split_ref.py), exactly: first pane, bounds, and the row list or
its absence.  T = the rows per workgroup tile of the streaming pass (csrc/panes.hpp kPaneTile): the sizes and seams below sit on it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pane_split_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = int(re.search(r"constexpr int kPaneTile = (\d+);", open(os.path.join(ROOT, "flock_amd", "csrc", "panes.hpp")).read()).group(1))
HOP = 5_000


@pytest.fixture(scope="module")
def gpu():
    from flock_amd import GpuContext
    ctx = GpuContext(0)
    yield ctx
    ctx.close()


def dev(arr, shift=0):
    """a device tensor of `arr`; shift: the [shift:] slice of a larger one (element-aligned only)"""
    import torch
    arr = np.ascontiguousarray(arr)
    whole = np.concatenate([np.full(shift, 0, arr.dtype), arr]) if shift else arr
    return torch.from_numpy(whole).to("cuda:0")[shift:]


def check(gpu, t, hop=HOP, origin=0, valid=None, max_panes=4096, shift=0, want_rows=None):
    t = np.asarray(t, np.int64)
    first, bounds, rows = ref.pane_split(t.tolist(), hop, origin, None if valid is None else valid.tolist(), max_panes)
    g_first, g_bounds, g_rows = gpu.pane_split(dev(t, shift), hop, origin, None if valid is None else dev(valid, 3 if shift else 0), max_panes)
    assert g_first == first and g_bounds.dtype == np.int64 and g_bounds.tolist() == bounds
    if want_rows is not None:
        assert (rows is not None) == want_rows
    if rows is None:
        assert g_rows is None
    else:
        assert g_rows is not None and g_rows.cpu().numpy().dtype == np.int32 and g_rows.cpu().tolist() == rows
    return first, bounds, rows


def ordered(n, panes=4, start=2 * HOP + 17):
    """n increasing timestamps over `panes` panes"""
    return start + (np.arange(n, dtype=np.int64) * panes * HOP) // max(n, 1)


@pytest.mark.parametrize("n", [0, 1, T - 1, T, T + 1, 3 * T + 5])
@pytest.mark.parametrize("shift", [0, 1])
def test_row_counts_around_the_tile(gpu, n, shift):
    first, bounds, _ = check(gpu, ordered(n), shift=shift, want_rows=False)
    assert bounds[-1] == n and (n == 0 or first == 2)
    check(gpu, ordered(n), valid=np.ones(n, np.uint8), shift=shift, want_rows=False)


@pytest.mark.parametrize("at", [T - 1, T, T + 1])
def test_the_pane_changes_at_the_tile_seam(gpu, at):
    n = 2 * T + 3
    t = np.where(np.arange(n) < at, 3 * HOP + np.arange(n) % HOP, 4 * HOP + np.arange(n) % HOP)
    first, bounds, _ = check(gpu, t, want_rows=False)
    assert (first, bounds) == (3, [0, at, n])


@pytest.mark.parametrize("shift", [0, 1])
def test_one_row_below_its_predecessor_across_the_seam(gpu, shift):
    """in pane order except that row T lies one pane below row T - 1 (the last row of one tile, the first of the next): the row list must appear"""
    n = 2 * T + 3
    t = np.full(n, 7 * HOP + 1, np.int64)
    t[T + shift] = 6 * HOP + 4_999
    t[T + shift + 1:] = 8 * HOP
    first, bounds, rows = check(gpu, t, shift=shift, want_rows=True)
    assert first == 6 and bounds == [0, 1, T + shift + 1, n] and rows[0] == T + shift
    # the same descent inside one pane breaks nothing
    t[T + shift] = 7 * HOP
    check(gpu, t, shift=shift, want_rows=False)


def test_timestamps_unordered_inside_panes(gpu):
    r = np.random.default_rng(5)
    n = 3 * T + 5
    pane = np.sort(r.integers(0, 6, n))
    check(gpu, pane * HOP + r.integers(0, HOP, n), want_rows=False)


def test_negative_timestamps_and_an_origin_above_every_row(gpu):
    n = T + 9
    t = -3 * HOP - 1 + (np.arange(n, dtype=np.int64) * 2 * HOP) // n             # from -15001 up: panes -4 .. -2
    first, _, _ = check(gpu, t, want_rows=False)
    assert first == -4
    first, _, _ = check(gpu, t, origin=10 * HOP + 3, want_rows=False)
    assert first < -10
    first, bounds, _ = check(gpu, np.array([-1, 0], np.int64), want_rows=False)   # t = origin - 1 lies in pane -1
    assert (first, bounds) == (-1, [0, 1, 2])


def test_empty_panes_in_between(gpu):
    n = T + 100
    t = np.where(np.arange(n) < 50, 2 * HOP, np.where(np.arange(n) < T + 1, 5 * HOP + 1, 9 * HOP))
    first, bounds, _ = check(gpu, t, want_rows=False)
    assert first == 2 and bounds == [0, 50, 50, 50, T + 1, T + 1, T + 1, T + 1, n]


def test_a_hop_of_one_millisecond(gpu):
    n = 3_000
    t = 1_600_000_000_000 + np.arange(n, dtype=np.int64) // 3
    first, bounds, _ = check(gpu, t, hop=1, want_rows=False)
    assert first == 1_600_000_000_000 and len(bounds) == 1_001


def test_all_rows_in_one_pane(gpu):
    r = np.random.default_rng(6)
    first, bounds, _ = check(gpu, 4 * HOP + r.integers(0, HOP, 2 * T + 1), want_rows=False)
    assert (first, bounds) == (4, [0, 2 * T + 1])


def test_a_shuffled_batch_gives_a_stable_row_list(gpu):
    r = np.random.default_rng(7)
    n = 3 * T + 5
    t = (1_000 + r.integers(0, 7, n)) * HOP + r.integers(0, HOP, n)
    t[:7] = (1_000 + np.arange(7)) * HOP                                          # (every one of the 7 panes is there)
    first, bounds, rows = check(gpu, t, want_rows=True)
    assert first == 1_000 and len(bounds) == 8
    ids = t // HOP
    for k in range(7):                                                            # stable: a pane's rows ascend
        mine = rows[bounds[k]:bounds[k + 1]]
        assert mine == sorted(mine) and (ids[mine] == 1_000 + k).all()
    check(gpu, t, valid=np.ones(n, np.uint8), shift=1, want_rows=True)


def refused(gpu, code, *args, **kw):
    from flock_amd import FlockGpuError, _ffi
    with pytest.raises(FlockGpuError) as e:
        gpu.pane_split(*args, **kw)
    assert e.value.code == getattr(_ffi, "ERR_" + code), str(e.value)
    return str(e.value)


@pytest.mark.parametrize("shift", [0, 1])
def test_a_null_timestamp_is_refused_and_named(gpu, shift):
    n = 2 * T + 40
    t = ordered(n)
    for rows in ([0], [T], [n - 1], [T, n - 1], [T - 1, T], [17, 5]):
        valid = np.ones(n, np.uint8)
        valid[rows] = 0
        with pytest.raises(ref.Refused) as e:
            ref.pane_split(t.tolist(), HOP, 0, valid.tolist())
        assert e.value.names == (min(rows),)
        msg = refused(gpu, "INVALID", dev(t, shift), HOP, 0, dev(valid, 3 if shift else 0))
        assert re.search(r"\brow %d\b" % min(rows), msg), msg
    check(gpu, t, valid=np.ones(n, np.uint8))                                     # the context still works


def test_more_panes_than_the_capacity_leave_the_bounds_untouched(gpu):
    from flock_amd import _ffi
    t = dev(ordered(T + 3, panes=6))
    first, bounds, _ = ref.pane_split(t.cpu().tolist(), HOP, 0)
    n_panes = len(bounds) - 1
    lib, sentinel = _ffi.load(), -77
    out = np.full(n_panes + 2, sentinel, np.int64)
    g_first, g_n, g_rows = C.c_int64(0), C.c_int32(0), C.c_void_p()

    def call(cap):
        return lib.flockgpu_pane_split(gpu._h, t.data_ptr(), None, t.numel(), 0, HOP, cap, C.byref(g_first), C.byref(g_n), out.ctypes.data_as(C.POINTER(C.c_int64)),
                                       C.byref(g_rows))
    assert call(n_panes - 1) == _ffi.ERR_UNSUPPORTED
    msg = lib.flockgpu_last_error(gpu._h).decode()
    assert (out == sentinel).all()
    for number in (first, first + n_panes - 1, n_panes - 1):
        assert re.search(r"(?<![\d-])%d\b" % number, msg), msg
    assert call(n_panes) == _ffi.OK and g_first.value == first and g_n.value == n_panes and not g_rows.value
    assert out[:n_panes + 1].tolist() == bounds and out[n_panes + 1] == sentinel
    out[:] = sentinel
    for bad_cap in (0, 65537):
        assert call(bad_cap) == _ffi.ERR_INVALID and (out == sentinel).all()
    # one garbage timestamp asks for billions of panes
    garbage = ordered(100)
    garbage[50] = 1 << 60
    refused(gpu, "UNSUPPORTED", dev(garbage), HOP)


def test_bad_arguments(gpu):
    t = dev(ordered(10))
    refused(gpu, "INVALID", t, 0)
    refused(gpu, "INVALID", t, -5)
    refused(gpu, "INVALID", dev(np.array([ref.INT64_MAX], np.int64)), 1, -1)      # pane 2^63 does not fit Int64
    first, bounds, _ = check(gpu, np.array([ref.INT64_MIN, ref.INT64_MAX], np.int64), hop=1 << 62, want_rows=False)
    assert (first, bounds) == (-2, [0, 1, 1, 1, 2])
