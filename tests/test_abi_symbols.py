"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol
include/flockgpu.h declares (no compute calls without a GPU)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from flock_amd import build
    build.build()
    from flock_amd import _ffi
    return _ffi.load()


def _declared():
    names = set()
    for hdr in ("flockgpu.h", "flockgpu_plan.h", "flockgpu_comm.h"):
        p = os.path.join(ROOT, "include", hdr)
        if os.path.exists(p):
            src = re.sub(r"/\*.*?\*/", "", open(p).read(), flags=re.S)
            names |= set(re.findall(r"\b(flockgpu_[a-z0-9_]+)\s*\(", src))
    return names


def test_every_declared_symbol_is_exported(lib):
    declared = _declared()
    assert len(declared) >= 20
    missing = [n for n in sorted(declared) if not hasattr(lib, n)]
    assert not missing, f"declared in include/*.h but not exported: {missing}"


def test_binding_table_matches_header(lib):
    from flock_amd import _ffi
    assert set(_ffi.SYMBOLS) <= _declared()
    assert lib.flockgpu_abi_version() == _ffi.ABI_VERSION


def test_product_never_imports_the_oracle():
    # a product path that routes through the oracle voids every parity claim
    pkg = os.path.join(ROOT, "flock_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "import oracle" not in src and "from oracle" not in src and "liboracle" not in src, f


def test_shipped_library_reads_no_environment():
    """Experiment knobs exist only in -DFLOCKGPU_EXPERIMENTAL builds (common.hpp exp_env): the one getenv of the kernels' sources sits
    under that switch, and the shipped library does not import the symbol at all."""
    import re
    import subprocess
    csrc = os.path.join(ROOT, "flock_amd", "csrc")
    uses = []
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".hpp", ".h")):
            for n, line in enumerate(open(os.path.join(csrc, f), errors="ignore"), 1):
                if re.search(r"(?<![_a-zA-Z])getenv\s*\(", line):
                    uses.append((f, n))
    assert [f for f, _ in uses] == ["common.hpp"], uses
    text = open(os.path.join(csrc, "common.hpp")).read()
    at = text.index("getenv(")
    assert "#ifdef FLOCKGPU_EXPERIMENTAL" in text[max(0, at - 400):at]
    so = os.path.join(ROOT, "flock_amd", "libflockgpu.so")
    if os.path.exists(so):
        dyn = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True).stdout
        assert not re.search(r"\bgetenv\b", dyn), "libflockgpu.so imports getenv"


def test_only_diagnostics_are_left_behind_exp_env():
    """The A/B variants of the kernel rounds are decided and gone (results: profiles/r02 .. r06): no source or tool names a
    define of the A/B family, and what exp_env() still reads in an experimental build are diagnostics, not selections between kernels."""
    kept = {"FLOCKGPU_GUARD_ARENA", "FLOCKGPU_GUARD_SLACK", "FLOCKGPU_GUARD_TRACE", "FLOCKGPU_PLAN_TIMES", "FLOCKGPU_RECORDED_EVENTS"}
    ab_family = "FLOCKGPU_" + "AB_"   # (spelled in two halves: a search of the tree for the prefix finds nothing, this file included)
    read = set()
    for top in (os.path.join(ROOT, "flock_amd", "csrc"), os.path.join(ROOT, "tools")):
        for dirpath, _, files in os.walk(top):
            for f in files:
                path = os.path.join(dirpath, f)
                src = open(path, errors="ignore").read()
                assert ab_family not in src, os.path.relpath(path, ROOT)
                if top.endswith("csrc"):
                    calls = re.findall(r"exp_env\(\s*([^)]*)\)", src)
                    names = [re.fullmatch(r'"(\w+)"', c.strip()) for c in calls if c.strip() not in ("const char *name", "const char *")]
                    assert all(names), (f, calls)   # every read names its variable literally
                    read |= {m.group(1) for m in names}
    assert read == kept, sorted(read ^ kept)


def test_counts_closed_form_matches_oracle():
    # host-only entry point (no GPU needed): event-kind counts of a stream slice
    import oracle
    from flock_amd import NEXMarkSource, Window
    for first in (0, 7, 49, 50, 12345):
        src = NEXMarkSource(3, 1000, Window.element_wise(), first_event_id=first)
        o = oracle.NexmarkStream(first_event_id=first, eps=1000)
        for n0, n1 in ((0, 0), (0, 1), (0, 50), (3, 997), (10, 3000)):
            assert src.counts(n0, n1) == o.counts(n0, n1)


def test_window_schedules_match_reference_launchers():
    import oracle
    from flock_amd import Window, window_epochs
    assert window_epochs(Window.element_wise(), 4) == oracle.elementwise_windows(4)
    assert window_epochs(Window.tumbling(10), 35) == oracle.tumbling_windows(35, 10) == [(0, 10), (10, 20), (20, 30)]
    assert window_epochs(Window.hopping(10, 5), 27) == oracle.hopping_windows(27, 10, 5) == [(0, 10), (5, 15), (10, 20), (15, 25)]
    # hopping.rs:40-45: seconds < window_size -> no window at all
    assert window_epochs(Window.hopping(10, 5), 7) == []


@pytest.mark.gpu
def test_one_hip_runtime_and_one_rccl_per_process():
    """libflockgpu.so is built by /opt/rocm's hipcc (RUNPATH /opt/rocm/lib), the PyTorch wheel bundles its own libamdhip64 / librccl
    under the SAME SONAMEs: whichever is mapped first serves both.  `_ffi.load()` imports torch first, so in a Python host the wheel's
    runtime is THE runtime (torch is the allocator and stream provider) -- one HIP runtime, one RCCL, whatever the import order the
    host used.  (A C host without torch resolves /opt/rocm's through the RUNPATH: tests/c_abi/consumer.c.)  DESIGN section 8."""
    import flock_amd
    from flock_amd import GpuContext
    flock_amd.load()
    c = GpuContext(0)
    c.close()
    maps = open("/proc/self/maps").read()
    for stem in ("libamdhip64.so", "librccl.so"):
        paths = {line.split()[-1] for line in maps.splitlines() if stem in line}
        assert len(paths) == 1, (stem, paths)
        assert "/torch/lib/" in next(iter(paths)), paths
