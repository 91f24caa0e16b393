"""CPU side of the surface entry points of the encode-time chain: the header declares the five prototypes after the AmtGpuSurfaces typedef,
the binding carries them, the built library exports them, the three Python methods exist, and the ABI version has not moved (additive)."""
import ctypes as C
import inspect
import os
import re
import subprocess

from amtlib import ROOT

PROTOTYPES = (
    "int amtgpu_erase_surfaces(AmtGpuErase* er, const AmtGpuSurfaces* batch, int nframes, const float* fades);",
    "int amtgpu_erase_surfaces_dfades(AmtGpuErase* er, const AmtGpuSurfaces* batch, int nframes, const float* d_fades);",
    "int amtgpu_erase_surfaces_dfades_to(AmtGpuErase* er, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes, const float* d_fades);",
    "int amtgpu_analyze_surfaces(AmtGpuAnalyze* an, const AmtGpuSurfaces* batch, int nframes, float* dout);",
    "int amtgpu_logoframe_scan_surfaces(AmtGpuLogoFrame* lf, const AmtGpuSurfaces* batch, int first, int nframes);",
)
NAMES = tuple(re.search(r"(amtgpu_\w+)\(", p).group(1) for p in PROTOTYPES)


def header():
    return open(os.path.join(ROOT, "include", "amt_gpu.h")).read()


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_declares_the_five_entry_points_after_the_typedef():
    hdr = squeeze(header())
    for proto in PROTOTYPES:
        assert squeeze(proto) in hdr, proto
    assert len(set(NAMES)) == 5
    raw = header()
    for name in NAMES:
        assert raw.index("} AmtGpuSurfaces;") < raw.index(name + "("), name
    # the descriptor's comment says that the const planes are written by the erase
    above = raw[raw.index("decoder surfaces: what a hardware decoder"):raw.index("typedef struct AmtGpuSurfaces")]
    assert "WRITE" in above and "amtgpu_erase_surfaces" in above
    # the shared scratch makes the luma entry points non re-entrant: the header says so
    assert raw.count("NOT re-entrant") >= 2


def test_abi_version_stays_5():
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", header(), re.M)


def test_binding_has_prototypes():
    from amatsukaze_amd import binding
    c_i, c_p = C.c_int, C.c_void_p
    want = {
        "amtgpu_erase_surfaces": (c_i, [c_p, c_p, c_i, c_p]),
        "amtgpu_erase_surfaces_dfades": (c_i, [c_p, c_p, c_i, c_p]),
        "amtgpu_erase_surfaces_dfades_to": (c_i, [c_p, c_p, c_p, c_i, c_p]),
        "amtgpu_analyze_surfaces": (c_i, [c_p, c_p, c_i, c_p]),
        "amtgpu_logoframe_scan_surfaces": (c_i, [c_p, c_p, c_i, c_i]),
    }
    assert set(want) == set(NAMES)
    for name, sig in want.items():
        assert binding.SIGNATURES[name] == sig, name


def test_python_methods_exist():
    import amatsukaze_amd as A
    sig = inspect.signature(A.AMTEraseLogo.erase_surfaces)
    assert list(sig.parameters) == ["self", "surfaces", "fades", "d_fades", "dst"]
    assert all(sig.parameters[k].default is None for k in ("fades", "d_fades", "dst"))
    sig = inspect.signature(A.AMTAnalyzeLogo.analyze_surfaces)
    assert list(sig.parameters) == ["self", "surfaces", "out"] and sig.parameters["out"].default is None
    assert list(inspect.signature(A.LogoFrame.scan_surfaces).parameters) == ["self", "surfaces", "first"]


def test_library_exports_them():
    from amatsukaze_amd import build as b
    b.build()
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    for f in NAMES:
        assert f in exported, f
