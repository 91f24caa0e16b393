"""ISA properties of the adaptive bob's decoder-surface kernels as build.py compiles them (CPU: hipcc cross-compiles gfx950): eight forms
-- interleaved {8-bit, 16-bit LSB, 16-bit MSB} x {16 bytes per lane, container by container} and planar MSB x the same two -- none with
scratch, spills, LDS traffic, AGPRs or atomics, all within 128 VGPRs (four waves per SIMD); the vector forms move 16 bytes per lane, issue
the 12 loads of an interpolated span together and take the horizontal neighbours from the neighbouring lanes' registers; the 8-bit
interleaved vector form keeps its arithmetic packed in 16-bit halves; the MSB vector forms shift packed, one v_pk_lshrrev_b16 per loaded
dword and one v_pk_lshlrev_b16 per stored one, and the LSB forms do not shift at all; the element forms touch single containers only."""
import re

import pytest

from test_isa_guards import kernels_of
from test_isa_surfaces import compile_file, lean

# template arguments <ES, VEC, MSB, IL> as they are mangled, and the VGPRs the compiler reports today (ROCm 7.2, -O3).  The budget is
# 128 = 4 waves per SIMD, as for the planar forms (106 / 51 / 75 / 57 there); the 16-bit forms ask the compiler for five waves per SIMD
# (at most 96 VGPRs), which their vector forms use
VGPR_TODAY = {"ILi1ELb1ELb0ELb1E": 120, "ILi1ELb0ELb0ELb1E": 60, "ILi2ELb1ELb0ELb1E": 89, "ILi2ELb0ELb0ELb1E": 61,
              "ILi2ELb1ELb1ELb1E": 88, "ILi2ELb0ELb1ELb1E": 60, "ILi2ELb1ELb1ELb0E": 84, "ILi2ELb0ELb1ELb0E": 56}
VGPR_BUDGET = 128
VGPR_FIVE_WAVES = 96
MSB = tuple(t for t in VGPR_TODAY if t[9:13] == "Lb1E")
VECTOR = tuple(t for t in VGPR_TODAY if t[5:9] == "Lb1E")
ELEMENT = tuple(t for t in VGPR_TODAY if t[5:9] == "Lb0E")
INTERLEAVED = tuple(t for t in VGPR_TODAY if t.endswith("Lb1E"))


@pytest.fixture(scope="module")
def kernels():
    asm = compile_file("render_adaptive_surface_kernels.hip")
    assert re.search(r"\.group_segment_fixed_size:\s+0\b", asm) and not re.search(r"\.group_segment_fixed_size:\s+[1-9]", asm)
    return kernels_of(asm)


def form(kernels, tag):
    (k,) = [k for n, k in kernels.items() if "kfm_render_adaptive_surfaces_kernel" + tag in n]
    return k


def test_eight_lean_forms(kernels):
    assert len(VECTOR) == 4 and len(ELEMENT) == 4 and len(INTERLEAVED) == 6
    assert len(kernels) == 8 and all("kfm_render_adaptive_surfaces_kernel" in n for n in kernels), sorted(kernels)
    for name, k in kernels.items():
        lean(name, k)
        assert not any(re.match(r"^\s*(global|buffer|flat)_atomic", l) for l in k["body"]), name
    for tag, today in VGPR_TODAY.items():
        m = form(kernels, tag)["meta"]
        print(tag, "VGPRs", m["vgpr_count"])
        assert m["agpr_count"] == 0 and m["vgpr_count"] <= VGPR_BUDGET, (tag, m)
        assert m["vgpr_count"] <= today + 8, (tag, m, "the figure in this file is out of date")
        if tag.startswith("ILi2E"):
            assert m["vgpr_count"] <= VGPR_FIVE_WAVES, (tag, m)


@pytest.mark.parametrize("tag", VECTOR)
def test_vector_forms_move_16_bytes_per_lane(kernels, tag):
    body = [l.strip() for l in form(kernels, tag)["body"]]
    loads = [i for i, l in enumerate(body) if l.startswith("global_load_dwordx4")]
    stores = [l for l in body if l.startswith("global_store_dwordx4")]
    # a kept or woven row: 1 load; an interpolated span: 12 per row function (interleaved: luma rows and UV rows) -- and one store each
    nfun = 2 if tag in INTERLEAVED else 1
    assert len(loads) == 1 + 12 * nfun and len(stores) == 1 + nfun, (len(loads), len(stores))
    waits = lambda i, j: [l for l in body[i:j] if l.startswith("s_waitcnt") and "vmcnt" in l]
    together = [k for k in range(len(loads) - 11) if not waits(loads[k], loads[k + 11])]
    assert together, "the 12 loads of a span are not issued together"
    if nfun == 2:
        assert max(together) - min(together) >= 12, "only one of the two row functions issues its 12 loads together"
    text = "\n".join(body)
    # the neighbours' edge dwords come over DPP wave shifts, U and D.  Unit step: one (8-bit) or two (16-bit) dwords from either side;
    # step 2 (interleaved chroma: six containers on either side): two (8-bit) or three (16-bit)
    es1 = tag.startswith("ILi1E")
    per_side = (1 if es1 else 2) + ((2 if es1 else 3) if tag in INTERLEAVED else 0)
    assert len(re.findall(r"v_mov_b32_dpp .*wave_shr:1", text)) == 2 * per_side
    assert len(re.findall(r"v_mov_b32_dpp .*wave_shl:1", text)) == 2 * per_side
    if es1:
        for ins in ("v_pk_sub_i16", "v_pk_max_i16", "v_pk_min_i16", "v_pk_add_u16", "v_pk_ashrrev_i16"):
            assert ins in text, ins
    else:
        # 17-bit differences: one container per register; nothing is packed but the shifts of the MSB forms: one per loaded dword of a
        # span (12 rows of 4) and per dword of the neighbouring lanes (U and D, 2 or 3 from either side), one per stored dword
        packed = re.findall(r"v_pk_\w+", text)
        nfun_dwords = [48 + 2 * 2 * 2] + ([48 + 2 * 2 * 3] if tag in INTERLEAVED else [])
        if tag in MSB:
            assert set(packed) == {"v_pk_lshrrev_b16", "v_pk_lshlrev_b16"}, sorted(set(packed))
            assert packed.count("v_pk_lshrrev_b16") == sum(nfun_dwords) and packed.count("v_pk_lshlrev_b16") == 4 * nfun, packed
        else:
            assert not packed, sorted(set(packed))


@pytest.mark.parametrize("tag", ELEMENT)
def test_element_forms_touch_containers_only(kernels, tag):
    text = "\n".join(form(kernels, tag)["body"])
    assert not re.search(r"global_(load|store)_dword", text) and "dpp" not in text
    assert ("global_load_ushort" in text and "global_store_short" in text) if tag.startswith("ILi2E") else "global_load_ushort" not in text
    assert "global_load_ubyte" in text and "global_store_byte" in text      # copies go byte by byte at either depth
    assert "v_pk_" not in text


def test_the_planar_file_still_holds_its_four_kernels_alone():
    ks = kernels_of(compile_file("render_adaptive_kernels.hip"))
    assert len(ks) == 4 and not any("surfaces" in n for n in ks), sorted(ks)
