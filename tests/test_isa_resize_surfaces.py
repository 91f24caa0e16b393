"""ISA properties of the resize kernels for decoder surfaces as build.py compiles them (CPU: hipcc cross-compiles gfx950), in the manner
of tests/test_isa_resize.py: the horizontal stage in sixteen forms ({NV12, interleaved LSB, P010-like, planar MSB} x {8, 12, 16 taps in
registers, table walk}) and the vertical stage in six ({8-bit, 16-bit LSB, 16-bit MSB} x {16-byte lanes, container by container}); none
with scratch or spills; the horizontal stage holds one 2 KiB region of LDS per wave and the vertical stage none; the vector forms move 16
bytes per access; no v_mul_lo_u32 anywhere; and a packed 16-bit shift in the MSB vector forms and in no LSB form.  Nothing else is
looked for."""
import re

import pytest

from test_isa_guards import kernels_of
from test_isa_surfaces import compile_file, lean

WAVES, REGION_BYTES = 4, 2048                    # kResizeWaves (csrc/kernels.hpp), kResizeRegionBytes (csrc/resize_region.h)
# VGPRs the compiler reports today (ROCm 7.2, -O3).  h: <container, taps, MSB, interleaved>; v: <container, 16-byte lanes, MSB>
VGPR_TODAY = {"h_kernelIhLi8ELb0ELb1E": 63, "h_kernelIhLi12ELb0ELb1E": 64, "h_kernelIhLi16ELb0ELb1E": 64, "h_kernelIhLi0ELb0ELb1E": 52,
              "h_kernelItLi8ELb0ELb1E": 42, "h_kernelItLi12ELb0ELb1E": 46, "h_kernelItLi16ELb0ELb1E": 50, "h_kernelItLi0ELb0ELb1E": 42,
              "h_kernelItLi8ELb1ELb1E": 42, "h_kernelItLi12ELb1ELb1E": 46, "h_kernelItLi16ELb1ELb1E": 50, "h_kernelItLi0ELb1ELb1E": 42,
              "h_kernelItLi8ELb1ELb0E": 38, "h_kernelItLi12ELb1ELb0E": 42, "h_kernelItLi16ELb1ELb0E": 46, "h_kernelItLi0ELb1ELb0E": 42,
              "v_kernelIhLb1ELb0E": 48, "v_kernelIhLb0ELb0E": 11, "v_kernelItLb1ELb0E": 32, "v_kernelItLb0ELb0E": 11,
              "v_kernelItLb1ELb1E": 32, "v_kernelItLb0ELb1E": 11}
VGPR_BUDGET = 64                                 # 8 waves per SIMD
H_FORMS = [t for t in VGPR_TODAY if t.startswith("h_")]
V_VECTOR = [t for t in VGPR_TODAY if re.match(r"v_kernelI.Lb1E", t)]
MSB = lambda tag: bool(re.match(r"h_kernelI.Li\d+ELb1E|v_kernelI.Lb.ELb1E", tag))
PACKED_SHIFTS = ("v_pk_lshrrev_b16", "v_pk_lshlrev_b16")


@pytest.fixture(scope="module")
def compiled():
    asm = compile_file("resize_surface_kernels.hip")
    lds = {}
    for m in re.finditer(r"- \.agpr_count:.*?\n(?=  - \.agpr_count:|\.\.\.|amdhsa\.target)", asm, re.S):
        lds[re.search(r"\.name:\s+(\S+)", m.group(0)).group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", m.group(0)).group(1))
    return kernels_of(asm), lds


def form(kernels, tag):
    (k,) = [k for n, k in kernels.items() if "resize_surface_" + tag in n]
    return k


def test_twenty_two_forms_without_scratch_or_spills(compiled):
    kernels, _ = compiled
    assert len(kernels) == 22 and all(sum("resize_surface_" + tag in n for tag in VGPR_TODAY) == 1 for n in kernels), sorted(kernels)
    assert len(H_FORMS) == 16 and len(V_VECTOR) == 3
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
        if "resize_surface_h_kernel" in name:
            assert lds[name] == WAVES * REGION_BYTES, (name, lds[name])
        else:
            assert lds[name] == 0, (name, lds[name])
            lean(name, k)                                                                      # ... and no LDS traffic either


def test_no_full_width_multiply_anywhere(compiled):
    kernels, _ = compiled
    for name, k in kernels.items():
        body = [l.strip() for l in k["body"]]
        assert not [l for l in body if l.startswith("v_mul_lo_u32")], name


@pytest.mark.parametrize("tag", H_FORMS)
def test_horizontal_forms_stage_16_bytes_per_lane(compiled, tag):
    body = [l.strip() for l in form(compiled[0], tag)["body"]]
    count = lambda ins: sum(l.startswith(ins) for l in body)
    assert count("ds_write_b128") == 1, count("ds_write_b128")
    # (the table walk also reads its coefficients four at a time)
    assert count("global_load_dwordx4") == (1 if "Li0E" not in tag else count("global_load_dwordx4")) >= 1


@pytest.mark.parametrize("tag", V_VECTOR)
def test_vertical_vector_forms_move_16_bytes_per_lane(compiled, tag):
    body = [l.strip() for l in form(compiled[0], tag)["body"]]
    count = lambda ins: sum(l.startswith(ins) for l in body)
    assert count("global_load_dwordx4") >= 1 and count("global_store_dwordx4") == 1, (count("global_load_dwordx4"), count("global_store_dwordx4"))


@pytest.mark.parametrize("tag", H_FORMS + V_VECTOR)
def test_a_packed_shift_per_dword_in_the_msb_vector_forms_and_none_in_the_lsb_ones(compiled, tag):
    body = [l.strip() for l in form(compiled[0], tag)["body"]]
    right, left = (sum(l.startswith(ins) for l in body) for ins in PACKED_SHIFTS)
    if not MSB(tag):
        assert right == 0 and left == 0, (tag, right, left)
    elif tag.startswith("h_"):
        assert right == 4 and left == 0, (tag, right, left)          # the four dwords of a staged 16 bytes, on the way in
    else:
        assert right == 0 and left == 4, (tag, right, left)          # the four dwords of a stored 16 bytes, on the way out
