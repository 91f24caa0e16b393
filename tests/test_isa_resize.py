"""ISA properties of the resize kernels as build.py compiles them (CPU: hipcc cross-compiles gfx950): the horizontal stage in eight forms
({8-bit, 16-bit containers} x {8, 12, 16 taps in registers, table walk}) and the vertical stage in four ({8-bit, 16-bit containers} x
{16-byte lanes, container by container}); none with scratch or spills in any form; the horizontal stage holds one 2 KiB region of LDS
per wave and the vertical stage none; the vector forms move 16 bytes per access; and no v_mul_lo_u32 anywhere -- the taps are 24-bit
multiply-adds, the addresses shifts, adds and scalar products.  Nothing else is looked for."""
import re

import pytest

from test_isa_guards import kernels_of
from test_isa_surfaces import compile_file, lean

WAVES, REGION_BYTES = 4, 2048                    # kResizeWaves (csrc/kernels.hpp), kResizeRegionBytes (csrc/resize_region.h)
# VGPRs the compiler reports today (ROCm 7.2, -O3)
VGPR_TODAY = {"resize_h_kernelIhLi8E": 57, "resize_h_kernelIhLi12E": 61, "resize_h_kernelIhLi16E": 64, "resize_h_kernelIhLi0E": 50,
              "resize_h_kernelItLi8E": 38, "resize_h_kernelItLi12E": 42, "resize_h_kernelItLi16E": 46, "resize_h_kernelItLi0E": 42,
              "resize_v_kernelIhLb1E": 48, "resize_v_kernelIhLb0E": 11, "resize_v_kernelItLb1E": 32, "resize_v_kernelItLb0E": 11}
VGPR_BUDGET = 64                                 # 8 waves per SIMD


@pytest.fixture(scope="module")
def compiled():
    asm = compile_file("resize_kernels.hip")
    lds = {}
    for m in re.finditer(r"- \.agpr_count:.*?\n(?=  - \.agpr_count:|\.\.\.|amdhsa\.target)", asm, re.S):
        lds[re.search(r"\.name:\s+(\S+)", m.group(0)).group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", m.group(0)).group(1))
    return kernels_of(asm), lds


def form(kernels, tag):
    (k,) = [k for n, k in kernels.items() if tag in n]
    return k


def test_twelve_forms_without_scratch_or_spills(compiled):
    kernels, _ = compiled
    assert len(kernels) == 12 and all(sum(tag in n for tag in VGPR_TODAY) == 1 for n in kernels), sorted(kernels)
    for name, k in kernels.items():
        m = k["meta"]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert not any("scratch_" in l for l in k["body"]), name
    for tag, today in VGPR_TODAY.items():
        m = form(kernels, tag)["meta"]
        assert m["agpr_count"] == 0 and m["vgpr_count"] <= VGPR_BUDGET, (tag, m)
        assert m["vgpr_count"] <= today + 8, (tag, m, "the figure in this file is out of date")


def test_lds_is_one_region_per_wave_in_the_horizontal_stage_and_none_in_the_vertical(compiled):
    kernels, lds = compiled
    for name, k in kernels.items():
        if "resize_h_kernel" in name:
            assert lds[name] == WAVES * REGION_BYTES, (name, lds[name])
        else:
            assert lds[name] == 0, (name, lds[name])
            lean(name, k)                                                                      # ... and no LDS traffic either


def test_no_full_width_multiply_anywhere(compiled):
    kernels, _ = compiled
    for name, k in kernels.items():
        body = [l.strip() for l in k["body"]]
        assert not [l for l in body if l.startswith("v_mul_lo_u32")], name


@pytest.mark.parametrize("tag", [t for t in VGPR_TODAY if "_h_" in t])
def test_horizontal_forms_stage_16_bytes_per_lane(compiled, tag):
    body = [l.strip() for l in form(compiled[0], tag)["body"]]
    count = lambda ins: sum(l.startswith(ins) for l in body)
    assert count("ds_write_b128") == 1, count("ds_write_b128")
    # (the table walk also reads its coefficients four at a time)
    assert count("global_load_dwordx4") == (1 if "Li0E" not in tag else count("global_load_dwordx4")) >= 1


@pytest.mark.parametrize("tag", ["resize_v_kernelIhLb1E", "resize_v_kernelItLb1E"])
def test_vertical_vector_forms_move_16_bytes_per_lane(compiled, tag):
    body = [l.strip() for l in form(compiled[0], tag)["body"]]
    count = lambda ins: sum(l.startswith(ins) for l in body)
    assert count("global_load_dwordx4") >= 1 and count("global_store_dwordx4") == 1, (count("global_load_dwordx4"), count("global_store_dwordx4"))
