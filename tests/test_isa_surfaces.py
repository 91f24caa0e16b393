"""ISA properties of the decoder-surface kernels as build.py compiles them (CPU: hipcc cross-compiles gfx950): the rectangle extraction
(surface_kernels.hip) is one kernel without scratch, spills or LDS that splits interleaved chroma with byte permutes and shifts MSB
samples with packed 16-bit shifts; the MSB form of the logo finder (logofind_msb_kernels.hip) keeps the plain 16-bit kernels' budget."""
import os
import re
import subprocess

import pytest

from test_isa_guards import CACHE, CSRC, kernels_of


def compile_file(name):
    from amatsukaze_amd import build as B
    flags = [f for f in B.FLAGS if f != "-fPIC"] + B.EXTRA_FLAGS.get(name, [])
    os.makedirs(CACHE, exist_ok=True)
    out = os.path.join(CACHE, f"{name}.{os.getpid()}.s")
    try:
        subprocess.check_call([B.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, name)], stderr=subprocess.DEVNULL)
        return open(out).read()
    finally:
        if os.path.exists(out):
            os.remove(out)


def lean(name, k):
    m = k["meta"]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    assert not any("scratch_" in l for l in k["body"]), name
    assert not any(re.match(r"^\s*ds_", l) for l in k["body"]), f"{name}: LDS traffic"
    assert not any(re.match(r"^\s*v_(mfma|smfmac)", l) for l in k["body"]), name


def test_extract_kernel_is_one_lean_kernel():
    asm = compile_file("surface_kernels.hip")
    ks = kernels_of(asm)
    assert len(ks) == 1 and "surfaces_extract_kernel" in next(iter(ks)), sorted(ks)
    (name, k), = ks.items()
    lean(name, k)
    assert re.search(r"\.group_segment_fixed_size:\s+0\b", asm)
    assert k["meta"]["vgpr_count"] + k["meta"]["agpr_count"] <= 64                       # 8 waves per SIMD
    body = "\n".join(k["body"])
    # 16-byte, 4-byte and sample-wide loads; the interleaved split stores 8 bytes per plane behind a 16-byte load
    for ins in ("global_load_dwordx4", "global_load_dword ", "global_load_ushort", "global_load_ubyte", "global_store_dwordx4",
                "global_store_dwordx2", "global_store_short", "global_store_byte"):
        assert ins in body, ins
    assert len(re.findall(r"v_perm_b32", body)) >= 8            # {U, V} x {bytes, half-words} of a 16-byte load: 2 permutes each
    assert "v_pk_lshrrev_b16" in body


def test_msb_finder_kernels_keep_the_16_bit_budget():
    ks = kernels_of(compile_file("logofind_msb_kernels.hip"))
    assert len(ks) == 2, sorted(ks)                             # {buffer, sample-wise} loads
    for name, k in ks.items():
        assert "logofind_kernelILi2E" in name and name.count("Lb1E") >= 1, name
        m = k["meta"]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert not any("scratch_" in l for l in k["body"]) and not any(re.match(r"^\s*ds_", l) for l in k["body"]), name
        assert m["vgpr_count"] + m["agpr_count"] <= 256, (name, m)
    buf = next(k for n, k in ks.items() if "ILi2ELb1ELb1E" in n)
    # the buffer-load form shifts packed: one v_pk_lshrrev_b16 per loaded dword (10 rows x 2 dwords, two row sets)
    assert sum("v_pk_lshrrev_b16" in l for l in buf["body"]) >= 20
