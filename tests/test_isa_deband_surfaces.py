"""ISA properties of the deband kernels for decoder surfaces as build.py compiles them (CPU: hipcc cross-compiles gfx950), in the manner of
tests/test_isa_deband.py: eight forms ({NV12, interleaved 16-bit LSB, P010-like, planar 16-bit MSB} x {16-byte lanes, container by
container}), none with scratch or spills, none with MFMA, atomics or a full-width 32-bit multiply; the staged tile's LDS is the constant
kernels.hpp derives for the planar kernel; the vector forms stage and store 16 bytes per lane; the MSB vector forms shift packed, one
16-bit right shift per staged dword and one left shift per stored dword, and the LSB forms hold no packed shift at all."""
import re

import pytest

from test_isa_deband import lds_bytes, lean_with_lds
from test_isa_guards import kernels_of
from test_isa_surfaces import compile_file

# <container, 16-byte lanes, MSB, interleaved>.  VGPRs the compiler reports today (ROCm 7.2, -O3); as in the planar kernel the vector forms
# hold ten staged 16-byte pieces in flight, and LDS, not registers, sets the occupancy
VGPR_TODAY = {"IhLb1ELb0ELb1E": 81, "ItLb1ELb0ELb1E": 74, "ItLb1ELb1ELb1E": 74, "ItLb1ELb1ELb0E": 73,
              "IhLb0ELb0ELb1E": 119, "ItLb0ELb0ELb1E": 75, "ItLb0ELb1ELb1E": 72, "ItLb0ELb1ELb0E": 73}
VGPR_BUDGET = 128                                                  # 4 waves per SIMD, as the planar kernel's
VECTOR = [t for t in VGPR_TODAY if re.match(r"I.Lb1E", t)]
NARROW = [t for t in VGPR_TODAY if re.match(r"I.Lb0E", t)]
MSB = lambda tag: bool(re.match(r"ItLb.ELb1E", tag))
INTERLEAVED = lambda tag: tag.endswith("Lb1E")
# row loops of a form: sample 0, and 1 and 2 with either blur_first; an interleaved form holds them twice, for the luma plane's cell and
# for the UV plane's, whose horizontal step is 2 containers
LOOPS = lambda tag: 10 if INTERLEAVED(tag) else 5


@pytest.fixture(scope="module")
def asm():
    return compile_file("deband_surface_kernels.hip")


@pytest.fixture(scope="module")
def kernels(asm):
    return kernels_of(asm)


def form(kernels, tag):
    (k,) = [k for n, k in kernels.items() if "deband_surface_kernel" + tag + "EEvNS" in n]
    return k


def test_eight_lean_forms(kernels):
    assert len(kernels) == 8 and all(sum("deband_surface_kernel" + tag + "EEvNS" in n for tag in VGPR_TODAY) == 1 for n in kernels), sorted(kernels)
    assert len(VECTOR) == 4 == len(NARROW) and sum(map(MSB, VGPR_TODAY)) == 4 and sum(map(INTERLEAVED, VGPR_TODAY)) == 6
    for name, k in kernels.items():
        lean_with_lds(name, k)
        assert not any(re.match(r"^\s*(global|buffer|flat|ds)_(atomic|add|sub|max|min|cmpst)", l) for l in k["body"]), name
    for tag, today in VGPR_TODAY.items():
        m = form(kernels, tag)["meta"]
        assert m["agpr_count"] == 0 and m["vgpr_count"] <= VGPR_BUDGET, (tag, m)
        assert m["vgpr_count"] <= today + 8, (tag, m, "the figure in this file is out of date")


def test_lds_is_the_planar_kernels(asm, kernels):
    sizes = {}
    for m in re.finditer(r"- \.agpr_count:.*?\n(?=  - \.agpr_count:|\.\.\.|amdhsa\.target)", asm, re.S):
        blk = m.group(0)
        sizes[re.search(r"\.name:\s+(\S+)", blk).group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
    assert set(sizes) == set(kernels)
    for name, size in sizes.items():
        es = 1 if "deband_surface_kernelIh" in name else 2
        assert size == lds_bytes(es) <= 65536, (name, size)


def test_no_kernel_holds_a_full_width_multiply(kernels):
    for name, k in kernels.items():
        body = [l.strip() for l in k["body"]]
        assert not [l for l in body if l.startswith("v_mul_lo_u32")], name
        # the references' addresses: dy * row + step * dx and dx * row - step * dy, 24-bit
        assert sum(l.startswith(("v_mul_i32_i24", "v_mad_i32_i24")) for l in body) >= 16, name


@pytest.mark.parametrize("tag", VECTOR)
def test_vector_forms_move_16_bytes_per_lane(kernels, tag):
    body = [l.strip() for l in form(kernels, tag)["body"]]
    count = lambda ins: sum(l.startswith(ins) for l in body)
    px, loops = (16 if tag.startswith("Ih") else 8), LOOPS(tag)
    # staging: ten 16-byte loads in flight, then their ten 16-byte LDS stores; one 16-byte store and one 16-byte read of a lane's centre
    # samples per row loop; its table entries: one vector load of dx and one of dy, the first step's and each loop's next step's
    assert count("ds_write_b128") == 10 and count("global_store_dwordx4") == loops == count("ds_read_b128")
    table = 2 + 2 * loops
    if px == 16:
        assert count("global_load_dwordx4") == 10 + table
    else:
        assert count("global_load_dwordx4") == 10 and count("global_load_dwordx2") >= table
    # the references: 1 + 2 + 2 + 4 + 4 per pixel over five loops, each one container wide
    assert count("ds_read_u8" if px == 16 else "ds_read_u16") == 13 * px * (loops // 5)
    assert count("s_barrier") == 2                                     # behind the staging, and in front of the next frame's


@pytest.mark.parametrize("tag", sorted(VGPR_TODAY))
def test_packed_shifts_in_the_msb_forms_and_none_in_the_lsb_ones(kernels, tag):
    body = [l.strip() for l in form(kernels, tag)["body"]]
    right, left = (sum(l.startswith(ins) for l in body) for ins in ("v_pk_lshrrev_b16", "v_pk_lshlrev_b16"))
    if not MSB(tag):
        assert right == 0 and left == 0, (tag, right, left)
    else:
        # out: the four dwords of a lane's 16 bytes in every row loop; in: the four dwords of each of the ten staged pieces (the narrow
        # forms stage container by container and shift each)
        assert left == 4 * LOOPS(tag), (tag, left)
        assert right == (40 if tag in VECTOR else 0), (tag, right)


@pytest.mark.parametrize("tag", NARROW)
def test_narrow_forms_touch_planes_container_by_container(kernels, tag):
    body = [l.strip() for l in form(kernels, tag)["body"]]
    text = "\n".join(body)
    assert not re.search(r"global_store_dwordx[234]", text) and "ds_write_b128" not in text
    if tag.startswith("It"):
        assert "global_load_ushort" in text and "global_store_short" in text and "global_load_ubyte" not in text
        assert not re.search(r"global_load_dwordx[34]", text)           # the only wide loads are the table's 8 bytes
    else:
        assert "global_load_ubyte" in text and "global_store_byte" in text
        # the only wide loads are the table's 16 bytes: dx and dy of the first step, and of the next step in each row loop
        assert sum(l.startswith("global_load_dwordx4") for l in body) == 2 + 2 * LOOPS(tag)
