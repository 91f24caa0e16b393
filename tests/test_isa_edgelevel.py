"""ISA properties of the edge level kernel as build.py compiles it (CPU: hipcc cross-compiles gfx950): four forms ({8-bit, 16-bit
containers} x {16-byte lanes, container by container}), none with a private segment, scratch or spills, none with LDS, MFMA or atomics;
the product of the rule is a 24-bit multiply and no kernel holds a full-width 32-bit one, on the vector unit or folded into a 64-bit
address; the 16-byte forms load and store 16 bytes per lane, take their neighbours' containers over DPP and compute 8-bit containers in
packed halves; the container-by-container forms hold no vector access at all."""
import re

import pytest

from test_isa_guards import kernels_of
from test_isa_surfaces import compile_file, lean

# VGPRs the compiler reports today (ROCm 7.2, -O3) for <uint8_t, vec>, <uint8_t, narrow>, <uint16_t, vec>, <uint16_t, narrow>.  The vector
# forms hold the window of five rows (30 dwords), the row requested ahead (6) and, at 8 bits, the rows taken apart into halves
VGPR_TODAY = {"IhLb1E": 125, "IhLb0E": 46, "ItLb1E": 86, "ItLb0E": 46}
# The occupancy the design needs: a wave's row costs it 600 to 900 vector instructions, 1 200 to 1 800 cycles of issue at two cycles each,
# and its one 16-byte load per row is requested a whole row ahead of its use, so a wave covers an HBM miss (about 900 cycles) by itself;
# what further waves are for is to keep the SIMD issuing while one waits at a strip's first rows or stores: three to a SIMD, 512 / 3
# registers rounded down to the allocation's step of 8
VGPR_BUDGET = 168
REPAIRS = 5                                                          # row loops per kernel: repair 0..4


@pytest.fixture(scope="module")
def asm():
    return compile_file("edgelevel_kernels.hip")


@pytest.fixture(scope="module")
def kernels(asm):
    return kernels_of(asm)


def form(kernels, tag):
    (k,) = [k for n, k in kernels.items() if "edgelevel_kernel" + tag in n]
    return k


def test_four_lean_forms(asm, kernels):
    assert len(kernels) == 4 and all("edgelevel_kernel" in n for n in kernels), sorted(kernels)
    for name, k in kernels.items():
        lean(name, k)                                                   # no private segment, no spill, no scratch, no LDS, no MFMA
        assert not any(re.match(r"^\s*(global|buffer|flat|ds)_(atomic|add|sub|max|min|cmpst)", l) for l in k["body"]), name
    assert [int(v) for v in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", asm)] == [0] * 4
    for tag, today in VGPR_TODAY.items():
        m = form(kernels, tag)["meta"]
        print(tag, m)
        assert m["agpr_count"] == 0 and m["vgpr_count"] <= VGPR_BUDGET, (tag, m)
        assert m["vgpr_count"] <= today + 8, (tag, m, "the figure in this file is out of date")


def test_no_kernel_holds_a_full_width_multiply(kernels):
    for name, k in kernels.items():
        body = [l.strip() for l in k["body"]]
        wide = [l for l in body if re.match(r"v_(mul_lo_[ui]32|mul_hi_[ui]32|mad_[ui]64_[ui]32)\b", l)]
        assert not wide, (name, wide[:3])
        # the rule's product, once per pixel and row loop
        px = (16 if "kernelIh" in name else 8) if "Lb1E" in name else 1
        assert sum(l.startswith("v_mul_i32_i24") for l in body) >= REPAIRS * px, name


@pytest.mark.parametrize("tag", ["IhLb1E", "ItLb1E"])
def test_vector_forms_move_16_bytes_per_lane(kernels, tag):
    body = [l.strip() for l in form(kernels, tag)["body"]]
    count = lambda ins: sum(l.startswith(ins) for l in body)
    # per row loop: the strip's first row and the row requested ahead, one 16-byte load each, and one 16-byte store; the chroma copy's pair
    assert count("global_load_dwordx4") == 2 * REPAIRS + 1 and count("global_store_dwordx4") == REPAIRS + 1
    # the neighbouring lanes' dwords: one from the left and one from the right per row that enters the window
    dpp = [l for l in body if l.startswith("v_mov_b32_dpp")]
    assert len(dpp) == 2 * REPAIRS and sum("wave_shr:1" in l for l in dpp) == REPAIRS == sum("wave_shl:1" in l for l in dpp), dpp[:2]
    if tag == "IhLb1E":
        # 8-bit containers in 16-bit halves: the ranges, the steps and the ranks are packed minima and maxima
        assert count("v_pk_max_i16") >= 100 * REPAIRS and count("v_pk_min_i16") >= 100 * REPAIRS and count("v_pk_sub_i16") >= 50 * REPAIRS
    else:
        # 16-bit containers one to a register: the ranks come from three-operand minima, maxima and medians -- repairs 2..4 take at least
        # two medians of sorted columns' rows per pixel (a column's own median is shared by the three pixels that read it)
        assert count("v_med3_i32") >= 8 * 2 * 3 and count("v_min3_") + count("v_max3_") >= 8 * 2 * REPAIRS


@pytest.mark.parametrize("tag", ["IhLb0E", "ItLb0E"])
def test_narrow_forms_touch_planes_container_by_container(kernels, tag):
    text = "\n".join(l.strip() for l in form(kernels, tag)["body"])
    assert not re.search(r"global_(load|store)_dwordx[234]", text) and "v_mov_b32_dpp" not in text
    if tag == "ItLb0E":
        assert "global_load_ushort" in text and "global_store_short" in text and "global_load_ubyte" not in text
    else:
        assert "global_load_ubyte" in text and "global_store_byte" in text
