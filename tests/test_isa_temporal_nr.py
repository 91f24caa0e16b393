"""ISA properties of the temporal noise reduction kernel as build.py compiles it (CPU: hipcc cross-compiles gfx950): four forms
({8-bit, 16-bit containers} x {16-byte lanes, container by container}), none with scratch, spills or LDS; the vector forms move 16
bytes of luma and 8 bytes of chroma per access; and no fused multiply-add anywhere -- the reference rounds the product, then the sum."""
import re

import pytest

from test_isa_guards import kernels_of
from test_isa_surfaces import compile_file, lean

# VGPRs the compiler reports today (ROCm 7.2, -O3): 214 / 44 / 100 / 50 for <uint8_t, vec>, <uint8_t, narrow>, <uint16_t, vec>,
# <uint16_t, narrow>.  The 8-bit vector form keeps a lane's 32 luma and 16 chroma sums, factors and centre samples in registers: 2 waves
# per SIMD, 256 registers being the most a wave can have
VGPR_TODAY = {"IhLb1E": 214, "IhLb0E": 44, "ItLb1E": 100, "ItLb0E": 50}
VGPR_BUDGET = 256


@pytest.fixture(scope="module")
def kernels():
    asm = compile_file("temporal_nr_kernels.hip")
    assert re.search(r"\.group_segment_fixed_size:\s+0\b", asm) and not re.search(r"\.group_segment_fixed_size:\s+[1-9]", asm)
    return kernels_of(asm)


def form(kernels, tag):
    (k,) = [k for n, k in kernels.items() if "temporal_nr_kernel" + tag in n]
    return k


def test_four_lean_forms(kernels):
    assert len(kernels) == 4 and all("temporal_nr_kernel" in n for n in kernels), sorted(kernels)
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


@pytest.mark.parametrize("tag", ["IhLb1E", "ItLb1E"])
def test_vector_forms_move_16_bytes_per_lane(kernels, tag):
    body = [l.strip() for l in form(kernels, tag)["body"]]
    count = lambda ins: sum(l.startswith(ins) for l in body)
    # the centre and the two walks of the window: two luma rows each; one store per luma row
    assert count("global_load_dwordx4") == 6 and count("global_store_dwordx4") == 2, (count("global_load_dwordx4"), count("global_store_dwordx4"))
    # ... and the U and V runs under them, 8 bytes each
    assert count("global_load_dwordx2") == 6 and count("global_store_dwordx2") == 2, (count("global_load_dwordx2"), count("global_store_dwordx2"))


@pytest.mark.parametrize("tag", ["IhLb0E", "ItLb0E"])
def test_narrow_forms_make_no_wide_access(kernels, tag):
    # (the compiler merges a lane's two luma containers into one access of twice the container, which the target allows unaligned; the
    # only 4-byte loads of the 8-bit form are the 1.f / count table's)
    text = "\n".join(form(kernels, tag)["body"])
    assert not re.search(r"global_(load|store)_dwordx[234]", text)
    if tag == "ItLb0E":
        assert "global_load_ushort" in text and "global_store_short" in text and "global_load_ubyte" not in text
    else:
        assert "global_load_ubyte" in text and "global_store_byte" in text and "global_store_dword" not in text
