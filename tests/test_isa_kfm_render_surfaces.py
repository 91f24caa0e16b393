"""ISA properties of the cadence renderer's decoder-surface kernels as build.py compiles them (CPU: hipcc cross-compiles gfx950): six
forms -- {8-bit, 16-bit containers} x {16 bytes per lane, container by container} for LSB containers, and {16 bytes per lane, container
by container} for MSB-aligned 16-bit ones -- none with scratch, spills, LDS or atomics, all within the planar kernel's register budget;
the vector forms move 16 bytes per lane; the MSB forms shift packed, the LSB forms do not shift at all."""
import re

import pytest

from test_isa_guards import kernels_of
from test_isa_surfaces import compile_file, lean

# template arguments <ES, VEC, MSB> as they are mangled, and the VGPRs the compiler reports today (ROCm 7.2, -O3).  The budget is
# 64 = 8 waves per SIMD, as for the planar forms (31 / 11 / 35 / 13 there): the two packed shifts of the MSB vector form cost no register
VGPR_TODAY = {"ILi1ELb1ELb0E": 31, "ILi1ELb0ELb0E": 11, "ILi2ELb1ELb0E": 35, "ILi2ELb0ELb0E": 13, "ILi2ELb1ELb1E": 35, "ILi2ELb0ELb1E": 16}
VGPR_BUDGET = 64
VECTOR = ("ILi1ELb1ELb0E", "ILi2ELb1ELb0E", "ILi2ELb1ELb1E")
MSB = ("ILi2ELb1ELb1E", "ILi2ELb0ELb1E")


@pytest.fixture(scope="module")
def kernels():
    asm = compile_file("render_surface_kernels.hip")
    assert re.search(r"\.group_segment_fixed_size:\s+0\b", asm) and not re.search(r"\.group_segment_fixed_size:\s+[1-9]", asm)
    return kernels_of(asm)


def form(kernels, tag):
    (k,) = [k for n, k in kernels.items() if "kfm_render_surfaces_kernel" + tag in n]
    return k


def test_six_lean_forms(kernels):
    assert len(kernels) == 6 and all("kfm_render_surfaces_kernel" in n for n in kernels), sorted(kernels)
    for name, k in kernels.items():
        lean(name, k)
        assert not any(re.match(r"^\s*(global|buffer|flat)_atomic", l) for l in k["body"]), name
    for tag, today in VGPR_TODAY.items():
        m = form(kernels, tag)["meta"]
        assert m["agpr_count"] == 0 and m["vgpr_count"] <= VGPR_BUDGET, (tag, m)
        assert m["vgpr_count"] <= today + 8, (tag, m, "the figure in this file is out of date")


@pytest.mark.parametrize("tag", VECTOR)
def test_vector_forms_move_16_bytes_per_lane(kernels, tag):
    body = [l.strip() for l in form(kernels, tag)["body"]]
    loads = [i for i, l in enumerate(body) if l.startswith("global_load_dwordx4")]
    stores = [l for l in body if l.startswith("global_store_dwordx4")]
    # a kept or woven row: 1 load; a line-average row: 2; a row with temporal neighbours: 4 -- and one store each, as in the planar kernel
    assert len(loads) == 7 and len(stores) == 3, (len(loads), len(stores))
    # the 4 loads of a temporal row are issued before the first of them is waited for
    waits = lambda i, j: [l for l in body[i:j] if l.startswith("s_waitcnt") and "vmcnt" in l]
    assert any(not waits(loads[k], loads[k + 3]) for k in range(len(loads) - 3)), "no 4 loads in flight together"
    text = "\n".join(body)
    assert "v_pk_max_u16" in text and "v_pk_min_u16" in text                 # |a - b| per 16-bit half
    assert len(re.findall(r"v_lerp_u8", text)) == (12 if tag.startswith("ILi1E") else 0)


@pytest.mark.parametrize("tag", sorted(VGPR_TODAY))
def test_only_the_msb_forms_shift_and_they_shift_packed(kernels, tag):
    text = "\n".join(form(kernels, tag)["body"])
    shr, shl = len(re.findall(r"v_pk_lshrrev_b16", text)), len(re.findall(r"v_pk_lshlrev_b16", text))
    if tag not in MSB:
        assert shr == 0 and shl == 0, (tag, shr, shl)
    elif tag in VECTOR:
        # per loaded dword of an interpolated row: 2 x 4 (line average) + 4 x 4 (with temporal neighbours); one left shift per stored dword
        assert shr >= 24 and shl >= 8, (tag, shr, shl)
    else:
        assert shr >= 6 and shl >= 2, (tag, shr, shl)                         # one container per lane: 2 + 4 loads, 2 stores


@pytest.mark.parametrize("tag", sorted(set(VGPR_TODAY) - set(VECTOR)))
def test_element_forms_touch_containers_only(kernels, tag):
    text = "\n".join(form(kernels, tag)["body"])
    assert not re.search(r"global_(load|store)_dword", text)
    assert ("global_load_ushort" in text and "global_store_short" in text) if tag.startswith("ILi2E") else "global_load_ushort" not in text
    assert "global_load_ubyte" in text and "global_store_byte" in text      # copies go byte by byte at either depth
