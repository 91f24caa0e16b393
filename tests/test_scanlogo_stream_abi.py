"""CPU side of the streamed ScanLogo session (amtgpu_scanlogo_stream_*): the header declares its seven entry points with the prototypes
the hosts were promised, the Python binding carries them, the built library exports them, and the ABI version has not moved (the
additions are additive)."""
import ctypes as C
import os
import re
import subprocess

from amtlib import ROOT

PROTOTYPES = (
    "AmtGpuScanLogoStream* amtgpu_scanlogo_stream_create(AmtGpuContext* ctx, int imgw, int imgh, int imgx, int imgy, int w, int h, "
    "int thy, int numMaxFrames);",
    "void amtgpu_scanlogo_stream_destroy(AmtGpuScanLogoStream* s);",
    "int amtgpu_scanlogo_stream_feed(AmtGpuScanLogoStream* s, const void* dY, const void* dU, const void* dV, int64_t strideY, "
    "int64_t strideUV, int pitchY, int pitchUV, int nframes, int* nkept, int* done);",
    "int amtgpu_scanlogo_stream_feed_rect(AmtGpuScanLogoStream* s, const void* dY, const void* dU, const void* dV, int64_t strideY, "
    "int64_t strideUV, int pitchY, int pitchUV, int nframes, int* nkept, int* done);",
    "int amtgpu_scanlogo_stream_status(const AmtGpuScanLogoStream* s, int64_t* nread, int* nkept, int* done);",
    "int amtgpu_scanlogo_stream_finish(AmtGpuScanLogoStream* s, int serviceid, const char* dstpath, AMTGPU_LOGO_ANALYZE_CB cb);",
    "int amtgpu_scanlogo_stream_finish_sharded(AmtGpuScanLogoStream* s, const AmtGpuCollectives* coll, int serviceid, "
    "const char* dstpath, AMTGPU_LOGO_ANALYZE_CB cb);",
)
NAMES = tuple(re.search(r"(amtgpu_\w+)\(", p).group(1) for p in PROTOTYPES)


def header():
    return open(os.path.join(ROOT, "include", "amt_gpu.h")).read()


def squeeze(text):
    """comments out, every run of white space one blank: a prototype may be wrapped and aligned any way the header likes"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_declares_the_seven_entry_points():
    hdr = squeeze(header())
    assert "typedef struct AmtGpuScanLogoStream AmtGpuScanLogoStream;" in hdr
    for proto in PROTOTYPES:
        assert squeeze(proto) in hdr, proto
    assert len(set(NAMES)) == 7


def test_sharded_finish_is_declared_after_the_collectives_struct():
    """plain C: the typedef name must be known where the prototype uses it"""
    hdr = header()
    assert hdr.index("} AmtGpuCollectives;") < hdr.index("amtgpu_scanlogo_stream_finish_sharded(")


def test_abi_version_stays_5():
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", header(), re.M)


def test_binding_has_prototypes():
    from amatsukaze_amd import binding
    c_i, c_p, c_i64, c_s = C.c_int, C.c_void_p, C.c_int64, C.c_char_p
    feed = (c_i, [c_p, c_p, c_p, c_p, c_i64, c_i64, c_i, c_i, c_i, c_p, c_p])
    want = {
        "amtgpu_scanlogo_stream_create": (c_p, [c_p] + [c_i] * 8),
        "amtgpu_scanlogo_stream_destroy": (None, [c_p]),
        "amtgpu_scanlogo_stream_feed": feed,
        "amtgpu_scanlogo_stream_feed_rect": feed,
        "amtgpu_scanlogo_stream_status": (c_i, [c_p] * 4),
        "amtgpu_scanlogo_stream_finish": (c_i, [c_p, c_i, c_s, binding.CB]),
        "amtgpu_scanlogo_stream_finish_sharded": (c_i, [c_p, c_p, c_i, c_s, binding.CB]),
    }
    assert set(want) == set(NAMES)
    for name, sig in want.items():
        assert binding.SIGNATURES[name] == sig, name


def test_python_mirror_is_exported():
    import amatsukaze_amd as A
    from amatsukaze_amd import sharding
    for name in ("ScanLogoStream", "ScanLogoAutoStream"):
        assert name in A.__all__ and callable(getattr(A, name))
    for method in ("feed", "feed_rect", "status", "finish", "__del__"):
        assert callable(getattr(A.ScanLogoStream, method))
    assert callable(sharding.scan_logo_stream_finish_sharded)


def test_library_exports_them():
    from amatsukaze_amd import build as b
    b.build()
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    for f in NAMES:
        assert f in exported, f
