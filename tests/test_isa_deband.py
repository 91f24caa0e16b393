"""ISA properties of the deband kernel as build.py compiles it (CPU: hipcc cross-compiles gfx950): four forms ({8-bit, 16-bit containers}
x {16-byte lanes, container by container}), none with scratch or spills; the staged tile's LDS is the constant kernels.hpp derives and
fits 64 KiB, so that two workgroups share a CU; the vector forms stage and store 16 bytes per lane and read a lane's centre samples with
one 16-byte LDS read; every reference is one container-wide LDS read whose address comes from 24-bit multiplies -- no kernel holds a
full-width 32-bit multiply.
(test_isa_surfaces.lean also refuses every LDS instruction, which this kernel is built on: lean_with_lds below is lean without that line.)"""
import re

import pytest

from test_isa_guards import kernels_of
from test_isa_surfaces import compile_file

# mirrored from csrc/kernels.hpp (tests/test_deband_host.py holds the two lines against the file)
TW, TH, HALO = 128, 96, 31


def lds_pitch(es):
    return ((TW + 2 * HALO) * es + 15 + 15) & ~15


def lds_bytes(es):
    return lds_pitch(es) * (TH + 2 * HALO)


# VGPRs the compiler reports today (ROCm 7.2, -O3): 82 / 119 / 74 / 74 for <uint8_t, vec>, <uint8_t, narrow>, <uint16_t, vec>,
# <uint16_t, narrow>; the vector forms hold ten staged 16-byte pieces in flight.  LDS, not registers, sets the occupancy: 2 workgroups of the 16-bit forms, 4 of the 8-bit ones per CU
VGPR_TODAY = {"IhLb1E": 82, "IhLb0E": 119, "ItLb1E": 74, "ItLb0E": 74}
VGPR_BUDGET = 128                                                  # 4 waves per SIMD: what 4 workgroups of 4 waves per CU need


@pytest.fixture(scope="module")
def asm():
    return compile_file("deband_kernels.hip")


@pytest.fixture(scope="module")
def kernels(asm):
    return kernels_of(asm)


def form(kernels, tag):
    (k,) = [k for n, k in kernels.items() if "deband_kernel" + tag in n]
    return k


def lean_with_lds(name, k):
    m = k["meta"]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    assert not any("scratch_" in l for l in k["body"]), name
    assert not any(re.match(r"^\s*v_(mfma|smfmac)", l) for l in k["body"]), name


def test_four_lean_forms(kernels):
    assert len(kernels) == 4 and all("deband_kernel" in n for n in kernels), sorted(kernels)
    for name, k in kernels.items():
        lean_with_lds(name, k)
        assert not any(re.match(r"^\s*(global|buffer|flat|ds)_(atomic|add|sub|max|min|cmpst)", l) for l in k["body"]), name
    for tag, today in VGPR_TODAY.items():
        m = form(kernels, tag)["meta"]
        assert m["agpr_count"] == 0 and m["vgpr_count"] <= VGPR_BUDGET, (tag, m)
        assert m["vgpr_count"] <= today + 8, (tag, m, "the figure in this file is out of date")


def test_the_staged_tile_fits_64_kib(asm, kernels):
    assert (lds_pitch(1), lds_pitch(2)) == (208, 400) and (lds_bytes(1), lds_bytes(2)) == (32864, 63200)
    sizes = {}
    for m in re.finditer(r"- \.agpr_count:.*?\n(?=  - \.agpr_count:|\.\.\.|amdhsa\.target)", asm, re.S):
        blk = m.group(0)
        sizes[re.search(r"\.name:\s+(\S+)", blk).group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
    assert set(sizes) == set(kernels)
    for name, size in sizes.items():
        es = 1 if "deband_kernelIh" in name else 2
        assert size == lds_bytes(es) <= 65536, (name, size)
    assert 2 * lds_bytes(2) <= 160 * 1024                              # two workgroups of the 16-bit form in a CU's LDS


def test_no_kernel_holds_a_full_width_multiply(kernels):
    for name, k in kernels.items():
        body = [l.strip() for l in k["body"]]
        assert not [l for l in body if l.startswith("v_mul_lo_u32")], name
        # the references' addresses: dy * row + dx and dx * row - dy, 24-bit
        assert sum(l.startswith(("v_mul_i32_i24", "v_mad_i32_i24")) for l in body) >= 16, name


@pytest.mark.parametrize("tag", ["IhLb1E", "ItLb1E"])
def test_vector_forms_move_16_bytes_per_lane(kernels, tag):
    body = [l.strip() for l in form(kernels, tag)["body"]]
    count = lambda ins: sum(l.startswith(ins) for l in body)
    px = 16 if tag.startswith("Ih") else 8
    # staging: ten 16-byte loads in flight, then their ten 16-byte LDS stores; one 16-byte store per row loop (sample 0, and 1 and 2
    # with either blur_first)
    assert count("ds_write_b128") == 10 and count("global_load_dwordx4") == (10 + 12 if px == 16 else 10)
    assert count("global_store_dwordx4") == 5, count("global_store_dwordx4")
    # a lane's centre samples: one 16-byte LDS read per row loop; its table entries: one vector load of dx and one of dy
    assert count("ds_read_b128") == 5, count("ds_read_b128")
    # (the first step's before anything is staged, the next step's inside each of the five loops)
    assert count("global_load_dwordx4" if px == 16 else "global_load_dwordx2") - (10 if px == 16 else 0) >= 12
    # the references: 1 + 2 + 2 + 4 + 4 per pixel over the five loops, each one container wide
    assert count("ds_read_u8" if px == 16 else "ds_read_u16") == 13 * px
    assert count("s_barrier") == 2                                     # behind the staging, and in front of the next frame's


@pytest.mark.parametrize("tag", ["IhLb0E", "ItLb0E"])
def test_narrow_forms_touch_planes_container_by_container(kernels, tag):
    body = [l.strip() for l in form(kernels, tag)["body"]]
    text = "\n".join(body)
    assert not re.search(r"global_store_dwordx[234]", text) and "ds_write_b128" not in text
    if tag == "ItLb0E":
        assert "global_load_ushort" in text and "global_store_short" in text and "global_load_ubyte" not in text
        assert not re.search(r"global_load_dwordx[34]", text)           # the only wide loads are the table's 8 bytes
    else:
        assert "global_load_ubyte" in text and "global_store_byte" in text
        # the only wide loads are the table's 16 bytes: dx and dy of the first step, and of the next step in each of the five row loops
        assert sum(l.startswith("global_load_dwordx4") for l in body) == 12
