"""CPU side of the monitored analysis mode (AMTGPU_ANALYZE_LINEAR_MONITORED): the header declares it, the Python binding and the built
library carry its entry points, and its kernels compile for gfx950 with the properties every kernel of eval_linear_kernels.hip keeps
(no scratch, no spills, no MFMA, no partial lgkmcnt wait with a scalar load outstanding)."""
import os
import re
import subprocess

import pytest

from amtlib import ROOT
from test_isa_guards import compile_asm, kernels_of, partial_waits_with_smem_outstanding, scratch_inside_loops

NEW_FUNCS = ("amtgpu_analyze_set_monitor", "amtgpu_analyze_monitor_stats")
NEW_KERNELS = ("analysis_sentinel_check_kernel", "analysis_iota_kernel", "analysis_mark_kernel")


def header():
    return open(os.path.join(ROOT, "include", "amt_gpu.h")).read()


def test_header_declares_the_mode_and_its_entry_points():
    hdr = header()
    assert re.search(r"^#define AMTGPU_ANALYZE_LINEAR_MONITORED 3\b", hdr, re.M)
    assert re.search(r"\bint\s+amtgpu_analyze_set_monitor\(AmtGpuAnalyze\* an, float tolerance, int sentinels\);", hdr)
    assert re.search(r"\bint\s+amtgpu_analyze_monitor_stats\(AmtGpuAnalyze\* an, float\* max_abs, int64_t\* frames_checked, int\* downgraded\);", hdr)
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", hdr, re.M)


def test_binding_has_prototypes():
    import ctypes as C
    from amatsukaze_amd import api, binding
    assert binding.SIGNATURES["amtgpu_analyze_set_monitor"] == (C.c_int, [C.c_void_p, C.c_float, C.c_int])
    assert binding.SIGNATURES["amtgpu_analyze_monitor_stats"] == (C.c_int, [C.c_void_p] * 4)
    assert api.AMTAnalyzeLogo.MODES["monitored"] == 3


def test_library_exports_them():
    from amatsukaze_amd import build as b
    b.build()
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    for f in NEW_FUNCS:
        assert f in exported, f


def test_filter_layer_forwards_the_mode():
    src = open(os.path.join(ROOT, "include", "amt_filters.hpp")).read()
    assert "AMTGPU_ANALYZE_LINEAR_MONITORED" in src and "amtgpu_analyze_monitor_stats" in src


@pytest.fixture(scope="module")
def linear_kernels():
    return kernels_of(compile_asm("eval_linear_kernels.hip"))


@pytest.mark.parametrize("kernel", NEW_KERNELS)
def test_monitor_kernels_isa(linear_kernels, kernel):
    found = [k for k in linear_kernels if kernel in k]
    assert len(found) == 1, (kernel, sorted(linear_kernels))
    k = linear_kernels[found[0]]
    m = k["meta"]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["agpr_count"] == 0 and m["vgpr_count"] <= 32, m
    assert not scratch_inside_loops(k["body"])
    assert not any("scratch_" in l for l in k["body"])
    assert not any(re.match(r"^\s*v_(mfma|smfmac)", l) for l in k["body"])
    hits, nblocks = partial_waits_with_smem_outstanding(k["body"])
    assert nblocks > 0 and not hits, hits[:3]
    # every write to memory is a vector (global / flat / LDS) instruction
    stores = [l.split()[0] for l in k["body"] if re.match(r"^\s*\S*(store|atomic)", l)]
    assert all(s.startswith(("global_", "flat_", "ds_", "buffer_")) for s in stores), stores
    if kernel == "analysis_sentinel_check_kernel":
        assert any(s.startswith("global_atomic_umax") for s in stores), stores       # max |diff| as float bits
