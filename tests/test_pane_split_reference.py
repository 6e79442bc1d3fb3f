"""Event-time panes on the host: the row-at-a-time reference of flockgpu_pane_split (tests/pane_split_ref.py) against numpy, the pane arithmetic
of csrc/panes.hpp as a stand-alone program, and the two new entry points in the headers, in _ffi and in the built library."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import pane_split_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", range(6))
def test_reference_equals_numpy_floor_divide_and_a_stable_argsort(seed):
    r = np.random.default_rng(1000 + seed)
    n = int(r.integers(1, 3000))
    hop = int(r.choice([1, 7, 1000, 5000]))
    origin = int(r.integers(-20_000, 20_000))
    panes = int(r.integers(1, 12))
    t = r.integers(origin - 3 * hop, origin - 3 * hop + panes * hop, n)
    if seed % 2 == 0:                                   # in pane order, timestamps inside a pane in any order
        t = t[np.argsort(np.floor_divide(t - origin, hop), kind="stable")]
    ids = np.floor_divide(t - origin, hop)
    first, bounds, rows = ref.pane_split(t.tolist(), hop, origin)
    assert first == int(ids.min()) and len(bounds) == int(ids.max() - ids.min()) + 2
    assert bounds == [int(np.searchsorted(np.sort(ids), first + k, side="left")) for k in range(len(bounds) - 1)] + [n]
    if (np.diff(ids) >= 0).all():
        assert rows is None
    else:
        assert rows == np.argsort(ids, kind="stable").tolist()


def test_reference_rounds_down_and_refuses():
    assert ref.pane_of(-1, 0, 5) == -1 and ref.pane_of(0, 0, 5) == 0 and ref.pane_of(4, 5, 5) == -1 and ref.pane_of(-5, 0, 5) == -1 and ref.pane_of(-6, 0, 5) == -2
    assert ref.pane_split([], 5) == (0, [0], None)
    assert ref.pane_split([12, 3, 12, 4], 5) == (0, [0, 2, 2, 4], [1, 3, 0, 2])          # an empty pane in between; stable
    assert ref.pane_split([3, 4, 12], 5) == (0, [0, 2, 2, 3], None)
    for args, code, names in [(([1], 0), "INVALID", ()), (([1, 2, 3], 5, 0, [1, 0, 0]), "INVALID", (1,)), (([0, 50], 5, 0, None, 10), "UNSUPPORTED", (0, 10, 10)),
                              (([ref.INT64_MAX], 1, -1), "INVALID", ())]:
        with pytest.raises(ref.Refused) as e:
            ref.pane_split(*args)
        assert (e.value.code, e.value.names) == (code, names)
    for p in (-3, 0, 4):
        assert ref.pane_of(ref.threshold(p, 17, 5), 17, 5) == p and ref.pane_of(ref.threshold(p, 17, 5) - 1, 17, 5) == p - 1


def test_both_entry_points_are_declared_bound_and_exported():
    from flock_amd import _ffi, build
    from flock_amd.runtime import ExecutionContext, _Plan
    public = open(os.path.join(ROOT, "include", "flockgpu.h")).read()
    plan = open(os.path.join(ROOT, "include", "flockgpu_plan.h")).read()
    assert re.search(r"\bint flockgpu_pane_split\(flockgpu_ctx \*ctx,", public)
    assert re.search(r"\bint flockgpu_plan_feed_pane_columns\(flockgpu_plan \*plan, int input, int64_t pane_id,", plan)
    assert len(_ffi.SYMBOLS["flockgpu_pane_split"][1]) == 11 and len(_ffi.SYMBOLS["flockgpu_plan_feed_pane_columns"][1]) == 7
    assert _ffi.ABI_VERSION == 1
    lib = C.CDLL(build.build())
    for name in ("flockgpu_pane_split", "flockgpu_plan_feed_pane_columns"):
        assert getattr(lib, name, None) is not None, name
    assert lib.flockgpu_abi_version() == 1
    assert "pane" in inspect.signature(ExecutionContext.feed_device_sources).parameters
    assert "pane" in inspect.signature(_Plan.feed_columns).parameters


def test_the_pane_arithmetic_on_the_host(tmp_path):
    """panes.hpp (the exact difference, the floor division, the threshold of a pane, the Int64 fit) as a stand-alone host program, under the address
    and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "panes_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "flock_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "panes_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "panes_test: ok" in out.stdout, out.stdout + out.stderr
