"""ISA properties of the adaptive bob's kernel as build.py compiles it (CPU: hipcc cross-compiles gfx950): four forms ({8-bit, 16-bit
containers} x {16 bytes per lane, container by container}), none with scratch, spills, LDS traffic, AGPRs or atomics, all within 128
VGPRs (four waves per SIMD); the vector forms move 16 bytes per lane, issue the 12 loads of an interpolated span together, take the
horizontal neighbours from the neighbouring lanes' registers and, at 8 bits, do the arithmetic packed in 16-bit halves."""
import re

import pytest

from test_isa_guards import kernels_of
from test_isa_surfaces import compile_file, lean

# VGPRs the compiler reports today (ROCm 7.2, -O3) for <1, vec>, <1, elem>, <2, vec>, <2, elem>.  The budget is 128 = 4 waves per SIMD
# for a kernel that keeps twelve 16-byte loads per lane in flight
VGPR_TODAY = {"ILi1ELb1E": 106, "ILi1ELb0E": 51, "ILi2ELb1E": 75, "ILi2ELb0E": 57}
VGPR_BUDGET = 128


@pytest.fixture(scope="module")
def kernels():
    asm = compile_file("render_adaptive_kernels.hip")
    assert re.search(r"\.group_segment_fixed_size:\s+0\b", asm) and not re.search(r"\.group_segment_fixed_size:\s+[1-9]", asm)
    return kernels_of(asm)


def form(kernels, tag):
    (k,) = [k for n, k in kernels.items() if "kfm_render_adaptive_kernel" + tag in n]
    return k


def test_four_lean_forms(kernels):
    assert len(kernels) == 4 and all("kfm_render_adaptive_kernel" in n for n in kernels), sorted(kernels)
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
    # a kept or woven row: 1 load; an interpolated span: 12 -- and one store each
    assert len(loads) == 13 and len(stores) == 2, (len(loads), len(stores))
    waits = lambda i, j: [l for l in body[i:j] if l.startswith("s_waitcnt") and "vmcnt" in l]
    assert any(not waits(loads[k], loads[k + 3]) for k in range(len(loads) - 3)), "no 4 loads in flight together"
    assert any(not waits(loads[k], loads[k + 11]) for k in range(len(loads) - 11)), "the 12 loads of a span are not issued together"
    text = "\n".join(body)
    # the neighbours' edge dwords come over DPP wave shifts: U and D, one (8-bit) or two (16-bit) dwords from either side
    assert len(re.findall(r"v_mov_b32_dpp .*wave_shr:1", text)) == 2 * (1 if tag == "ILi1ELb1E" else 2)
    assert len(re.findall(r"v_mov_b32_dpp .*wave_shl:1", text)) == 2 * (1 if tag == "ILi1ELb1E" else 2)
    if tag == "ILi1ELb1E":
        for ins in ("v_pk_sub_i16", "v_pk_max_i16", "v_pk_min_i16", "v_pk_add_u16", "v_pk_ashrrev_i16"):
            assert ins in text, ins
    else:
        assert "v_pk_" not in text                                         # 17-bit differences: one container per register


@pytest.mark.parametrize("tag", ["ILi1ELb0E", "ILi2ELb0E"])
def test_element_forms_touch_containers_only(kernels, tag):
    text = "\n".join(form(kernels, tag)["body"])
    assert not re.search(r"global_(load|store)_dword", text) and "dpp" not in text
    assert ("global_load_ushort" in text and "global_store_short" in text) if tag == "ILi2ELb0E" else "global_load_ushort" not in text
    assert "global_load_ubyte" in text and "global_store_byte" in text      # copies go byte by byte at either depth
