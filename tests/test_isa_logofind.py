"""ISA properties of the logo finder's kernel (logofind_kernels.hip) as build.py compiles it: no scratch, no MFMA, a VGPR budget per
sample width, and every scalar-memory instruction a load -- the kernel writes only through vector memory instructions."""
import os
import re
import subprocess

import pytest

from test_isa_guards import CACHE, CSRC, kernels_of

# budgets (VGPRs): 8-bit samples keep 3 waves per SIMD (512 / 168), 16-bit samples -- twice the row registers -- 2 (512 / 256)
BUDGET = {1: 168, 2: 256}


def compile_logofind():
    from amatsukaze_amd import build as B
    src = os.path.join(CSRC, "logofind_kernels.hip")
    flags = [f for f in B.FLAGS if f != "-fPIC"] + B.EXTRA_FLAGS.get("logofind_kernels.hip", [])
    os.makedirs(CACHE, exist_ok=True)
    out = os.path.join(CACHE, f"logofind_kernels.{os.getpid()}.s")
    try:
        subprocess.check_call([B.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, src], stderr=subprocess.DEVNULL)
        return open(out).read()
    finally:
        if os.path.exists(out):
            os.remove(out)


@pytest.fixture(scope="module")
def kernels():
    ks = kernels_of(compile_logofind())
    assert len(ks) == 4, sorted(ks)            # {8, 16}-bit samples x {buffer, sample-wise} loads
    return ks


def test_no_scratch_no_mfma(kernels):
    for name, k in kernels.items():
        m = k["meta"]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        # (the sample-wise fallback for unpadded ragged rows parks a few scalars in VGPR lanes -- v_writelane, no memory; the buffer-load
        # form every padded or 4-sample-aligned frame takes has none)
        if "Lb1E" in name:
            assert m["sgpr_spill_count"] == 0, (name, m)
        assert not any("scratch_" in l for l in k["body"]), name
        assert not any(re.match(r"^\s*v_(mfma|smfmac)", l) for l in k["body"]), name
        assert not any(re.match(r"^\s*ds_", l) for l in k["body"]), f"{name}: LDS traffic"


def test_vgpr_budget(kernels):
    for name, k in kernels.items():
        es = int(re.search(r"logofind_kernelILi(\d)", name).group(1))
        m = k["meta"]
        assert m["vgpr_count"] + m["agpr_count"] <= BUDGET[es], (name, m["vgpr_count"], m["agpr_count"])


def test_scalar_memory_is_loads_only(kernels):
    for name, k in kernels.items():
        smem = [l.strip() for l in k["body"] if re.match(r"^\s*s_\w*(load|store|atomic|dcache|scratch)", l)]
        assert smem, name                                     # (the kernel arguments come in through scalar loads)
        bad = [l for l in smem if not re.match(r"^s_(load|buffer_load)_", l)]
        assert not bad, f"{name}: scalar-memory instructions other than loads: {bad[:4]}"
        # the accumulators are flushed with vector 64-bit atomics
        assert any(re.match(r"^\s*(global|buffer|flat)_atomic_add_(x2|u64)", l) for l in k["body"]), name
