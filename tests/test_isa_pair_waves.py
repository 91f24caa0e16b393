"""Resource guards of the scan pair kernel's second shape (csrc/eval_pair1_duo_kernels.hip: 7 + 1 waves, compiled for four waves per SIMD so
that two workgroups share a CU).  CPU side: hipcc cross-compiles gfx950 without a GPU, with build.py's flags (the helper and the cache of
test_isa_scan_units.py).  Only the code object's metadata is read:

  * at most 128 VGPRs -- four waves per SIMD -- and no AGPRs;
  * no vector or scalar spills, no scratch;
  * max_flat_workgroup_size 512 = (7 + 1) x 64: what the launcher asks for.
"""
import re

import pytest

import test_isa_scan_units as SU

SRC = "eval_pair1_duo_kernels.hip"
KERNELS = ["logo_eval_pair1_duo_kernelIhE", "logo_eval_pair1_duo_kernelItE", "logo_eval_pair1_duo_ldexp_kernelIhE", "logo_eval_pair1_duo_ldexp_kernelItE"]
FIELDS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "max_flat_workgroup_size")


@pytest.fixture(scope="module")
def metadata():
    """{mangled kernel name: {field: value}} of the file's amdhsa.kernels entries"""
    asm = SU.compile_asm(SRC)
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?\n(?=  - \.agpr_count:|\.\.\.|amdhsa\.target)", asm, re.S):
        blk = m.group(0)
        out[re.search(r"\.name:\s+(\S+)", blk).group(1)] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) for k in FIELDS}
    return out


def test_the_file_holds_the_four_instances(metadata):
    assert len(metadata) == 4 and all(sum(k in n for n in metadata) == 1 for k in KERNELS), sorted(metadata)


@pytest.mark.parametrize("sub", KERNELS)
def test_four_waves_per_simd(metadata, sub):
    (m,) = [v for n, v in metadata.items() if sub in n]
    print(sub, m)
    assert m["vgpr_count"] <= 128 and m["agpr_count"] == 0
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0
    assert m["max_flat_workgroup_size"] == 512
