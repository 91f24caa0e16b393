"""CPU side of the decoder-surface entry points: the header declares the AmtGpuSurfaces descriptor and the four entry points that take it
(or, for the MSB weave, the weave's own argument list), the ctypes mirror has the header's layout, the binding carries the prototypes,
the built library exports them, and the ABI version has not moved (the additions are additive)."""
import ctypes as C
import os
import re
import subprocess

from amtlib import ROOT

PROTOTYPES = (
    "int amtgpu_surfaces_extract_rect(AmtGpuContext* ctx, const AmtGpuSurfaces* src, int imgx, int imgy, int w, int h, int nframes, "
    "void* dY, void* dU, void* dV, int64_t dstrideY, int64_t dstrideUV, int dpitchY, int dpitchUV);",
    "int amtgpu_scanlogo_stream_feed_surfaces(AmtGpuScanLogoStream* s, const AmtGpuSurfaces* batch, int nframes, int* nkept, int* done);",
    "int amtgpu_logofind_add_surfaces(AmtGpuLogoFind* lf, const AmtGpuSurfaces* batch, int nframes);",
    "int amtgpu_weave_fields_batch_msb(AmtGpuContext* ctx, const void* dsrcY, const void* dsrcU, const void* dsrcV, int64_t src_strideY, "
    "int64_t src_strideUV, int src_pitchY, int src_pitchUV, int num_pictures, const int* top_index, const int* bottom_index, int nv12, "
    "int bits, int width, int height, void* dY, void* dU, void* dV, int64_t strideY, int64_t strideUV, int pitchY, int pitchUV, int nframes);",
)
NAMES = tuple(re.search(r"(amtgpu_\w+)\(", p).group(1) for p in PROTOTYPES)

# the descriptor as the issue states it: (C type, name) in order
FIELDS = (("const void*", "Y"), ("const void*", "U"), ("const void*", "V"), ("int64_t", "strideY"), ("int64_t", "strideUV"), ("int", "pitchY"),
          ("int", "pitchUV"), ("int", "bits"), ("int", "interleaved"), ("int", "msb_aligned"), ("int", "reserved"))
CTYPE = {"const void*": C.c_void_p, "int64_t": C.c_int64, "int": C.c_int}


def header():
    return open(os.path.join(ROOT, "include", "amt_gpu.h")).read()


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def header_fields():
    """(type, name) of every member of AmtGpuSurfaces as the header declares them (a declaration may name several members)"""
    body = re.search(r"typedef struct AmtGpuSurfaces \{(.*?)\} AmtGpuSurfaces;", squeeze(header())).group(1)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const void\*|int64_t|int)\s*(.+)$", decl)
        assert m, decl
        out += [(m.group(1), n.strip()) for n in m.group(2).split(",")]
    return tuple(out)


def test_header_declares_the_descriptor_and_the_four_entry_points():
    hdr = squeeze(header())
    assert header_fields() == FIELDS
    for proto in PROTOTYPES:
        assert squeeze(proto) in hdr, proto
    assert len(set(NAMES)) == 4
    # plain C: the typedef is known where the prototypes use it
    raw = header()
    for name in NAMES[:3]:
        assert raw.index("} AmtGpuSurfaces;") < raw.index(name + "("), name


def test_ctypes_mirror_has_the_headers_layout():
    from amatsukaze_amd import binding

    class Want(C.Structure):
        _fields_ = [(n, CTYPE[t]) for t, n in header_fields()]

    got = binding.Surfaces
    assert [(n, t) for n, t in got._fields_] == [(n, t) for n, t in Want._fields_]
    assert C.sizeof(got) == C.sizeof(Want) == 64
    for n, _ in Want._fields_:
        assert getattr(got, n).offset == getattr(Want, n).offset, n


def test_abi_version_stays_5():
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", header(), re.M)


def test_binding_has_prototypes():
    from amatsukaze_amd import binding
    c_i, c_p, c_i64 = C.c_int, C.c_void_p, C.c_int64
    want = {
        "amtgpu_surfaces_extract_rect": (c_i, [c_p, c_p] + [c_i] * 5 + [c_p] * 3 + [c_i64, c_i64, c_i, c_i]),
        "amtgpu_scanlogo_stream_feed_surfaces": (c_i, [c_p, c_p, c_i, c_p, c_p]),
        "amtgpu_logofind_add_surfaces": (c_i, [c_p, c_p, c_i]),
        "amtgpu_weave_fields_batch_msb": binding.SIGNATURES["amtgpu_weave_fields_batch"],
    }
    assert set(want) == set(NAMES)
    for name, sig in want.items():
        assert binding.SIGNATURES[name] == sig, name


def test_python_mirror_is_exported():
    import inspect
    import amatsukaze_amd as A
    for name in ("DeviceSurfaces", "extract_rect"):
        assert name in A.__all__ and callable(getattr(A, name))
    assert callable(A.ScanLogoStream.feed_surfaces) and callable(A.LogoFinder.add_surfaces)
    assert inspect.signature(A.weave_fields).parameters["msb"].default is False
    s = A.DeviceSurfaces(None, None, width=64, height=40)
    assert (s.V, s.bits, s.interleaved, s.msb) == (None, 8, False, False)


def test_library_exports_them():
    from amatsukaze_amd import build as b
    b.build()
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    for f in NAMES:
        assert f in exported, f
