"""ISA properties of the surface erase kernel as build.py compiles it (CPU: hipcc cross-compiles gfx950): erase_surface_kernels.hip holds
delogo_surfaces_kernel instantiations only, each without scratch, spills, LDS traffic or MFMA and in an occupancy class no lower than
delogo_kernel's of the same container size (erase_scan_kernels.hip, compiled here), and the 16-bit one shifts packed."""
import re

from test_isa_guards import kernels_of
from test_isa_surfaces import compile_file, lean


def waves_per_simd(meta):
    """waves a SIMD of gfx950 holds at this register count: 512 VGPRs (arch + acc, allocated in blocks of 8) per lane, 8 waves at most"""
    regs = meta["vgpr_count"] + meta["agpr_count"]
    return min(8, 512 // max(8, (regs + 7) // 8 * 8))


def test_surface_erase_kernels_are_lean_and_keep_delogos_occupancy():
    asm = compile_file("erase_surface_kernels.hip")
    ks = kernels_of(asm)
    assert len(ks) == 2 and all("delogo_surfaces_kernel" in n for n in ks), sorted(ks)
    assert len(re.findall(r"\.group_segment_fixed_size:\s+0\b", asm)) == 2
    base = {n: k for n, k in kernels_of(compile_file("erase_scan_kernels.hip")).items() if "delogo_kernel" in n}
    assert len(base) == 2, sorted(base)
    for tag in ("Ih", "It"):                                  # uint8_t, uint16_t containers
        (name, k), = [(n, k) for n, k in ks.items() if f"delogo_surfaces_kernel{tag}E" in n]
        (bname, bk), = [(n, k) for n, k in base.items() if f"delogo_kernel{tag}E" in n]
        lean(name, k)
        assert waves_per_simd(k["meta"]) >= waves_per_simd(bk["meta"]), (name, k["meta"], bk["meta"])
    (k16,) = [k for n, k in ks.items() if "delogo_surfaces_kernelItE" in n]
    assert any(re.match(r"^\s*v_pk_(lshrrev|lshlrev)_b16", l) for l in k16["body"])
