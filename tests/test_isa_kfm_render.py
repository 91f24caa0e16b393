"""ISA properties of the cadence renderer's kernel as build.py compiles it (CPU: hipcc cross-compiles gfx950): four forms ({8-bit,
16-bit containers} x {16 bytes per lane, container by container}), none with scratch, spills or LDS; the vector forms move 16 bytes per
lane, issue an interpolated row's loads together and do the arithmetic packed."""
import re

import pytest

from test_isa_guards import kernels_of
from test_isa_surfaces import compile_file, lean

# VGPRs the compiler reports today (ROCm 7.2, -O3): 31 / 11 / 35 / 13 for <1, vec>, <1, elem>, <2, vec>, <2, elem>.  The budget below is
# 64 = 8 waves per SIMD, the occupancy an HBM-bound copy wants: 29 registers of headroom over the largest form
VGPR_TODAY = {"ILi1ELb1E": 31, "ILi1ELb0E": 11, "ILi2ELb1E": 35, "ILi2ELb0E": 13}
VGPR_BUDGET = 64


@pytest.fixture(scope="module")
def kernels():
    asm = compile_file("render_kernels.hip")
    assert re.search(r"\.group_segment_fixed_size:\s+0\b", asm) and not re.search(r"\.group_segment_fixed_size:\s+[1-9]", asm)
    return kernels_of(asm)


def form(kernels, tag):
    (k,) = [k for n, k in kernels.items() if "kfm_render_kernel" + tag in n]
    return k


def test_four_lean_forms(kernels):
    assert len(kernels) == 4 and all("kfm_render_kernel" in n for n in kernels), sorted(kernels)
    for name, k in kernels.items():
        lean(name, k)
        assert not any(re.match(r"^\s*(global|buffer|flat)_atomic", l) for l in k["body"]), name
    for tag, today in VGPR_TODAY.items():
        m = form(kernels, tag)["meta"]
        assert m["agpr_count"] == 0 and m["vgpr_count"] <= VGPR_BUDGET, (tag, m)
        assert m["vgpr_count"] <= today + 8, (tag, m, "the figure in this file is out of date")


@pytest.mark.parametrize("tag", ["ILi1ELb1E", "ILi2ELb1E"])
def test_vector_forms_move_16_bytes_per_lane(kernels, tag):
    body = [l.strip() for l in form(kernels, tag)["body"]]
    loads = [i for i, l in enumerate(body) if l.startswith("global_load_dwordx4")]
    stores = [l for l in body if l.startswith("global_store_dwordx4")]
    # a kept or woven row: 1 load; a line-average row: 2; a row with temporal neighbours: 4 -- and one store each
    assert len(loads) == 7 and len(stores) == 3, (len(loads), len(stores))
    # the 4 loads of a temporal row are issued before the first of them is waited for
    waits = lambda i, j: [l for l in body[i:j] if l.startswith("s_waitcnt") and "vmcnt" in l]
    assert any(not waits(loads[k], loads[k + 3]) for k in range(len(loads) - 3)), "no 4 loads in flight together"
    text = "\n".join(body)
    assert "v_pk_max_u16" in text and "v_pk_min_u16" in text                 # |a - b| per 16-bit half
    if tag == "ILi1ELb1E":
        assert len(re.findall(r"v_lerp_u8", text)) == 12                     # (a + b + 1) >> 1 of 4 bytes: 4 dwords x {spatial, spatial + temporal}
    else:
        assert "v_lerp_u8" not in text


@pytest.mark.parametrize("tag", ["ILi1ELb0E", "ILi2ELb0E"])
def test_element_forms_touch_containers_only(kernels, tag):
    text = "\n".join(form(kernels, tag)["body"])
    assert not re.search(r"global_(load|store)_dword", text)
    assert ("global_load_ushort" in text and "global_store_short" in text) if tag == "ILi2ELb0E" else "global_load_ushort" not in text
    assert "global_load_ubyte" in text and "global_store_byte" in text      # copies go byte by byte at either depth
