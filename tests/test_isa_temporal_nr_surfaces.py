"""ISA properties of the temporal noise reduction on decoder surfaces as build.py compiles it (CPU: hipcc cross-compiles gfx950): eight
forms ({NV12, interleaved LSB, P010 / P012, planar MSB} x {16-byte lanes, container by container}), none with scratch, spills, LDS or
atomics; the interleaved vector forms move a lane's chroma as ONE 16-byte run of the UV row; the MSB forms shift packed; and no fused
multiply-add anywhere -- the reference rounds the product, then the sum."""
import re

import pytest

from test_isa_guards import kernels_of
from test_isa_surfaces import compile_file, lean

# <T, VEC, MSB, IL> as the symbol spells it
NV12_VEC, NV12_NARROW = "IhLb1ELb0ELb1E", "IhLb0ELb0ELb1E"
IL16_VEC, IL16_NARROW = "ItLb1ELb0ELb1E", "ItLb0ELb0ELb1E"
P010_VEC, P010_NARROW = "ItLb1ELb1ELb1E", "ItLb0ELb1ELb1E"
PMSB_VEC, PMSB_NARROW = "ItLb1ELb1ELb0E", "ItLb0ELb1ELb0E"
# VGPRs the compiler reports today (ROCm 7.2, -O3).  The NV12 vector form has 16-byte luma lanes like the planar 8-bit kernel (214
# there): a lane's 32 luma and 16 chroma sums, factors and centre samples stay in registers, 2 waves per SIMD, no scratch
VGPR_TODAY = {NV12_VEC: 247, NV12_NARROW: 39, IL16_VEC: 110, IL16_NARROW: 45, P010_VEC: 81, P010_NARROW: 46, PMSB_VEC: 86, PMSB_NARROW: 50}
VGPR_BUDGET = 256


@pytest.fixture(scope="module")
def kernels():
    asm = compile_file("temporal_nr_surface_kernels.hip")
    assert re.search(r"\.group_segment_fixed_size:\s+0\b", asm) and not re.search(r"\.group_segment_fixed_size:\s+[1-9]", asm)
    return kernels_of(asm)


def form(kernels, tag):
    (k,) = [k for n, k in kernels.items() if "temporal_nr_surfaces_kernel" + tag in n]
    return k


def test_eight_lean_forms(kernels):
    assert len(kernels) == 8 and all("temporal_nr_surfaces_kernel" in n for n in kernels), sorted(kernels)
    for name, k in kernels.items():
        lean(name, k)
        assert not any(re.match(r"^\s*(global|buffer|flat)_atomic", l) for l in k["body"]), name
    for tag, today in VGPR_TODAY.items():
        m = form(kernels, tag)["meta"]
        assert m["agpr_count"] == 0 and m["vgpr_count"] <= VGPR_BUDGET, (tag, m)
        assert m["vgpr_count"] <= today + 8, (tag, m, "the figure in this file is out of date")


def test_no_fused_multiply_add_in_any_form(kernels):
    for name, k in kernels.items():
        body = [l.strip() for l in k["body"]]
        fused = [l for l in body if re.match(r"v_(pk_)?(fma|fmac|mad|mac)_(f32|legacy_f32|f16)", l)]
        assert not fused, (name, fused[:3])
        assert any(l.startswith("v_mul_f32") or l.startswith("v_pk_mul_f32") for l in body), name      # the product is rounded ...
        assert any(l.startswith("v_add_f32") or l.startswith("v_pk_add_f32") for l in body), name      # ... and then the sum


@pytest.mark.parametrize("tag", [NV12_VEC, IL16_VEC, P010_VEC])
def test_interleaved_vector_forms_move_three_16_byte_runs(kernels, tag):
    body = [l.strip() for l in form(kernels, tag)["body"]]
    count = lambda ins: sum(l.startswith(ins) for l in body)
    # the centre and the two walks of the window: two luma rows and the UV run under them each; one store per row
    assert count("global_load_dwordx4") == 9 and count("global_store_dwordx4") == 3, (count("global_load_dwordx4"), count("global_store_dwordx4"))
    assert not re.search(r"global_(load|store)_dwordx[23]", "\n".join(body))


def test_the_planar_msb_vector_form_moves_what_the_planar_kernel_moves(kernels):
    body = [l.strip() for l in form(kernels, PMSB_VEC)["body"]]
    count = lambda ins: sum(l.startswith(ins) for l in body)
    assert count("global_load_dwordx4") == 6 and count("global_store_dwordx4") == 2, (count("global_load_dwordx4"), count("global_store_dwordx4"))
    assert count("global_load_dwordx2") == 6 and count("global_store_dwordx2") == 2, (count("global_load_dwordx2"), count("global_store_dwordx2"))


@pytest.mark.parametrize("tag", [P010_VEC, PMSB_VEC])
def test_msb_vector_forms_shift_packed(kernels, tag):
    body = [l.strip() for l in form(kernels, tag)["body"]]
    count = lambda ins: sum(l.startswith(ins) for l in body)
    # 12 dwords per window frame, loaded at three places; 12 dwords stored
    assert count("v_pk_lshrrev_b16") >= 36 and count("v_pk_lshlrev_b16") >= 12, (count("v_pk_lshrrev_b16"), count("v_pk_lshlrev_b16"))


@pytest.mark.parametrize("tag", [NV12_NARROW, IL16_NARROW, P010_NARROW, PMSB_NARROW])
def test_narrow_forms_make_no_wide_access(kernels, tag):
    # (the compiler merges a lane's two neighbouring containers -- two luma columns, or the U and the V of a pair -- into one access of
    # twice the container, which the target allows unaligned, as it does in the planar kernel's narrow forms; so an interleaved narrow
    # form is left with no access of one container.  The only 4-byte loads of the 8-bit form are the 1.f / count table's)
    text = "\n".join(form(kernels, tag)["body"])
    assert not re.search(r"global_(load|store)_dwordx[234]", text)
    widths = set(re.findall(r"global_(?:load|store)_(\w+)", text))
    if tag == NV12_NARROW:
        assert widths <= {"ubyte", "byte", "ushort", "short", "dword"} and "global_store_dword" not in text, widths
    elif tag == PMSB_NARROW:
        assert "global_load_ushort" in text and "global_store_short" in text and widths <= {"ushort", "short", "dword"}, widths
    else:
        assert widths <= {"ushort", "short", "dword"}, widths
