"""ISA properties of the frame metrics' MSB form (stats_msb_kernels.hip) as build.py compiles it: three kernels, no scratch, no spills, no
MFMA, no LDS traffic, the plain frame_stats_kernel's register budget, and the packed 16-bit shift."""
import os
import re
import subprocess

import pytest

from test_isa_guards import CACHE, CSRC, kernels_of

BUDGET = 256            # VGPRs + AGPRs: two waves per SIMD, the budget of frame_stats_kernel (test_isa_guards.FILES)


def compile_stats_msb():
    from amatsukaze_amd import build as B
    src = os.path.join(CSRC, "stats_msb_kernels.hip")
    flags = [f for f in B.FLAGS if f != "-fPIC"] + B.EXTRA_FLAGS.get("stats_msb_kernels.hip", [])
    os.makedirs(CACHE, exist_ok=True)
    out = os.path.join(CACHE, f"stats_msb_kernels.{os.getpid()}.s")
    try:
        subprocess.check_call([B.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, src], stderr=subprocess.DEVNULL)
        return open(out).read()
    finally:
        if os.path.exists(out):
            os.remove(out)


@pytest.fixture(scope="module")
def kernels():
    ks = kernels_of(compile_stats_msb())
    assert len(ks) == 3, sorted(ks)            # buffer loads, buffer loads with ragged rows, plain loads -- 16-bit containers only
    assert all(re.search(r"frame_stats_kernelILi2ELb[01]ELb[01]ELb1EEE", n) for n in ks), sorted(ks)      # <ES 2, ., ., MSB true>
    return ks


def test_no_scratch_no_spills_no_mfma_no_lds(kernels):
    for name, k in kernels.items():
        m = k["meta"]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert not any("scratch_" in l for l in k["body"]), name
        assert not any(re.match(r"^\s*v_(mfma|smfmac)", l) for l in k["body"]), name
        assert not any(re.match(r"^\s*ds_", l) for l in k["body"]), f"{name}: LDS traffic"


def test_vgpr_budget(kernels):
    for name, k in kernels.items():
        m = k["meta"]
        assert m["vgpr_count"] + m["agpr_count"] <= BUDGET, (name, m["vgpr_count"], m["agpr_count"])


def test_packed_16_bit_shift(kernels):
    for name, k in kernels.items():
        assert any(re.match(r"^\s*v_pk_lshrrev_b16", l) for l in k["body"]), name
