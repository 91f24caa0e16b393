"""CPU side of the frame metrics on decoder surfaces: the header declares the two entry points, the binding carries their prototypes, the
built library exports them, FrameStats and sharding have the methods, the ABI version has not moved -- and the inputs of
tests/test_gpu_surface_stats.py can tell the right kernel from two wrong ones (a condition on the inputs, checked here in numpy)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import surface_stats_clips as S
from amtlib import ROOT

PROTOTYPES = (
    "int amtgpu_framestats_surfaces(AmtGpuFrameStats* fs, const AmtGpuSurfaces* batch, const AmtGpuSurfaces* prev, int nframes, uint64_t* dout);",
    "int amtgpu_framestats_sharded_surfaces(AmtGpuFrameStats* fs, const AmtGpuCollectives* coll, const AmtGpuSurfaces* batch, "
    "const AmtGpuSurfaces* prev, int first, int nlocal, int num_frames, uint64_t* metrics_out);",
)
NAMES = tuple(re.search(r"(amtgpu_\w+)\(", p).group(1) for p in PROTOTYPES)


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def header():
    return open(os.path.join(ROOT, "include", "amt_gpu.h")).read()


def test_header_declares_the_entry_points():
    hdr, raw = squeeze(header()), header()
    for proto, name in zip(PROTOTYPES, NAMES):
        assert squeeze(proto) in hdr, proto
        assert raw.index("} AmtGpuSurfaces;") < raw.index(name + "("), name          # plain C: the typedef is known where it is used
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", raw, re.M)                    # additions only
    # both block comments that list who takes surfaces name the new entry points
    assert raw.count("amtgpu_framestats_surfaces") >= 3


def test_binding_has_prototypes():
    from amatsukaze_amd import binding
    c_i, c_p = C.c_int, C.c_void_p
    assert binding.SIGNATURES["amtgpu_framestats_surfaces"] == (c_i, [c_p, c_p, c_p, c_i, c_p])
    assert binding.SIGNATURES["amtgpu_framestats_sharded_surfaces"] == (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p])


def test_library_exports_them():
    from amatsukaze_amd import build as b
    assert "stats_msb_kernels.hip" in b.SOURCES
    b.build()
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    for f in NAMES:
        assert f in exported, f


def test_python_methods():
    import amatsukaze_amd as A
    from amatsukaze_amd import sharding
    assert list(inspect.signature(A.FrameStats.run_device_surfaces).parameters) == ["self", "surfaces", "out", "prev"]
    assert list(inspect.signature(A.FrameStats.run_surfaces).parameters) == ["self", "surfaces", "prev"]
    assert list(inspect.signature(sharding.framestats_sharded_surfaces).parameters) == ["fs", "surfaces", "first", "num_frames", "coll", "prev"]
    for fn in (A.FrameStats.run_device_surfaces, A.FrameStats.run_surfaces, sharding.framestats_sharded_surfaces):
        assert inspect.signature(fn).parameters["prev"].default is None


# ---- the GPU test's inputs, judged without a GPU ----
def test_case_list_reaches_every_form_depth_height_and_batch_length():
    import plane_edge_clips as P
    for f, (W, pitch) in S.FORMS.items():
        assert P.predicted_form("frame_stats", W, pitch, 2) == f
    assert set(S.FORMS) == {"buf", "buf_ragged", "plain"}
    for f in S.FORMS:
        geo = [c for c in S.GEOMETRY_CASES if c[0] == f]
        assert {c[1] for c in geo} == {9, 10, 12, 15}
        assert {c[2] for c in geo} == {4, 16, 21, 33} | ({9} if f == "plain" else set())
        assert {c[3] for c in S.BATCH_CASES if c[0] == f} == {1, 2, 33, 65}
        assert {c[1] for c in S.LOW_BITS_CASES if c[0] == f} == {9, 10, 12, 15}


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_inputs_tell_the_right_kernel_from_two_wrong_ones(case):
    """a 32-bit shift of packed dwords without per-half handling, and the plain kernel on unshifted containers with its sums shifted
    afterwards: both must give other records than the oracle on every run of every case"""
    f, bits, H, N, kind = case
    shift = 16 - bits
    clip, sep = S.clip_of(case)
    low = clip.frames() & ((1 << shift) - 1)
    assert np.all(low != 0)                                        # non-zero low bits under every sample
    if kind == "alternating":
        s = clip.frames() >> shift
        assert np.all(low == (1 << shift) - 1) and set(np.unique(s)) == {0, (1 << bits) - 1} and np.all(s[:, :, 1:] != s[:, :, :-1])
    assert np.all(clip.buf[clip.base + clip.W:clip.base + clip.pitch] == 0xFFFF)           # poison: row padding ...
    assert np.all(clip.buf[clip.base + clip.H * clip.pitch:clip.base + clip.frame_stride] == 0xFFFF)      # ... and the gap between surfaces
    for batch, prev in S.runs_of(case):
        want = S.truth(batch, prev, bits)
        for wrong in (S.wrong_shift32, S.wrong_shifted_sums):
            got = wrong(batch, prev, bits)
            assert np.any(got != want, axis=1).all(), (wrong.__name__, S.case_id(case))      # every frame's record shows it
