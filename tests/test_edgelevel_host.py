"""CPU side of the edge level (amtgpu_edgelevel; DESIGN.md section 6g, "parity unpinned"): the numpy restatement (tests/edgelevel_ref.py)
against the rule's known answers and against planted pixels on every boundary of the rule and one beyond; that the soft clip of the GPU
tests is worth running; the lane rule against its definition (tests/cpp/edgelevel_lane_rule_test.cpp, plain g++); the entry point in
the header, the binding and the library; the kernel's constants that the GPU and ISA tests mirror."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import edgelevel_ref as R
from amtlib import ROOT

CSRC = os.path.join(ROOT, "amatsukaze_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")

DEPTHS = [(8, 8), (14, 14), (16, 16)]
SOFT_SIZES = [(40, 12), (1058, 12), (546, 40), (40, 70)]


def dt_of(bits):
    return np.uint8 if bits <= 8 else np.uint16


def centre(s, bits, strength=16, threshold=10, repair=0):
    m = s.shape[0] // 2
    return int(R.filter_plane(s, bits, strength, threshold, repair)[m, m])


# ---- the known answers of the issue's table ----
EDGE = [200, 200, 200, 190, 120, 50, 40, 40, 40, 40]
LEVELLED = [200, 200, 200, 200, 120, 40, 40, 40, 40, 40]


@pytest.mark.parametrize("r", [0, 1, 2])
def test_known_answer_the_soft_edge_is_levelled(r):
    s = np.tile(np.array(EDGE, np.uint8), (10, 1))
    out = R.filter_plane(s, 8, 16, 10, r)
    assert out[5].tolist() == LEVELLED
    assert out[2:8].tolist() == [LEVELLED] * 6 and out[:2].tolist() == [EDGE] * 2 == out[8:].tolist()      # the border rows stay


def test_known_answer_repair_4_takes_it_back():
    s = np.tile(np.array(EDGE, np.uint8), (10, 1))
    assert np.array_equal(R.filter_plane(s, 8, 16, 10, 4), s)


def test_known_answer_transposed_takes_the_vertical_line():
    s = np.tile(np.array(EDGE, np.uint8), (10, 1)).T.copy()
    out = R.filter_plane(s, 8, 16, 10, 2)
    assert out[:, 5].tolist() == LEVELLED
    k = R.classify(s, 8, 10)
    assert k["vertical"][k["levelled"]].all() and k["levelled"].any()


@pytest.mark.parametrize("r", range(5))
def test_known_answer_ramp_and_step_stay(r):
    ramp = np.tile(np.arange(0, 250, 25, dtype=np.uint8), (10, 1))
    assert np.array_equal(R.filter_plane(ramp, 8, 16, 10, r), ramp) and R.classify(ramp, 8, 10)["blurred"].all()
    step = np.tile(np.array([40] * 5 + [200] * 5, np.uint8), (10, 1))
    k = R.classify(step, 8, 10)
    assert np.array_equal(R.filter_plane(step, 8, 16, 10, r), step) and (k["sharp"] | k["flat"]).all() and k["sharp"].any()


# ---- whole planes ----
@pytest.mark.parametrize("depth", DEPTHS, ids=lambda d: "bits%d" % d[0])
def test_constant_planes_threshold_32767_and_planes_without_interior_copy(depth):
    bits, content = depth
    dt = dt_of(bits)
    for v in (0, 1, (1 << content) - 1):
        s = np.full((12, 40), v, dt)
        for r in range(5):
            assert np.all(R.filter_plane(s, bits, 255, 0, r) == v)
    rnd = R.clip(40, 12, depth, "random")[0][0]
    assert not np.array_equal(R.filter_plane(rnd, bits), rnd)
    for r in range(5):
        assert np.array_equal(R.filter_plane(rnd, bits, 255, 32767, r), rnd)                  # T = 32767 << (bits - 8) is no less than any range
    for h, w in ((4, 4), (4, 40), (12, 4), (2, 2)):
        tiny = np.random.default_rng(bits).integers(0, 1 << content, (h, w)).astype(dt)
        assert np.array_equal(R.filter_plane(tiny, bits, 255, 0, 2), tiny)
    # the border of a plane with an interior stays
    out = R.filter_plane(rnd, bits, 255, 0, 0)
    frame = np.ones(rnd.shape, bool)
    frame[2:-2, 2:-2] = False
    assert np.array_equal(out[frame], rnd[frame]) and not np.array_equal(out, rnd)


def test_chroma_is_untouched():
    planes = R.clip(40, 12, (8, 8), "random")
    Y, U, V = R.filter_clip(planes, 8, 255, 0, 2)
    assert np.array_equal(U, planes[1]) and np.array_equal(V, planes[2]) and not np.array_equal(Y, planes[0])
    # frames are independent
    for f in range(planes[0].shape[0]):
        assert np.array_equal(Y[f], R.filter_plane(planes[0][f], 8, 255, 0, 2))


# ---- planted pixels ----
@pytest.mark.parametrize("vertical", [False, True])
@pytest.mark.parametrize("bits", [8, 14, 16])
def test_planted_pixels_on_each_boundary_and_one_beyond(bits, vertical):
    for name, (line, changes) in R.boundary_lines(bits).items():
        s = R.planted_line(line, vertical, dt=dt_of(bits))
        got = centre(s, bits)
        assert (got != line[2]) == changes, (name, bits, line, got)
        k = R.classify(s, bits, 10)
        m = s.shape[0] // 2 - 2
        assert bool(k["vertical"][m, m]) == vertical and bool(k["levelled"][m, m]) == changes, name


def test_a_tie_takes_the_horizontal_line():
    s = R.planted_line([50, 50, 61, 90, 90])                            # levelled: 61 -> 52
    s[2:7, 4] = [61, 61, 61, 101, 101]                                  # rv = 40 = rh, a step that is sharp
    assert centre(s, 8) == 52
    s[5:7, 4] = 102                                                     # rv = 41: the vertical line, sharp: kept
    assert centre(s, 8) == 61


def test_the_shift_floors_and_both_clamps_hold():
    s = R.planted_line([50, 50, 54, 61, 61])                            # avg 55, c - avg = -1
    assert centre(s, 8, strength=8) == 53                               # (-1 * 8) >> 4 = -1, not 0
    assert centre(s, 8, strength=7) == 53 and centre(s, 8, strength=0) == 54
    assert centre(s, 8, strength=255) == 50                             # 54 - 16 = 38, clamped to mn
    assert centre(R.planted_line([50, 50, 58, 61, 61]), 8, strength=255) == 61      # 58 + 47, clamped to mx
    assert centre(R.planted_line([50, 50, 56, 61, 61]), 8, strength=8) == 56        # (1 * 8) >> 4 = 0


def test_every_repair_on_a_3x3_with_duplicates():
    for line, want in (([50, 50, 54, 61, 61], [50, 50, 50, 54, 54]), ([50, 50, 58, 61, 61], [61, 61, 60, 58, 54])):
        s = R.planted_line(line, base=54)
        s[3, 3:6] = [54, 54, 60]
        s[5, 3:6] = [40, 54, 54]
        # the nine, sorted: 40 50 54 54 54 54 c' 60 61 with c' = 54 or 58 in its place
        assert [centre(s, 8, 255, 10, r) for r in range(5)] == want, line
    # repair moves a pixel that the level left at c: strength 0
    s = R.planted_line([50, 50, 54, 61, 61], base=54)
    s[3, 3:6] = 60
    s[5, 3:6] = 60
    assert centre(s, 8, 0, 10, 0) == 54 and centre(s, 8, 0, 10, 4) == 60


def test_0_and_65535_side_by_side():
    s = R.planted_line([0, 0, 20000, 65535, 65535], dt=np.uint16)
    assert centre(s, 16, 16, 10) == 7233 and centre(s, 16, 255, 10) == 0
    s = R.planted_line([0, 0, 45535, 65535, 65535], dt=np.uint16)
    assert centre(s, 16, 255, 10) == 65535 and centre(s, 16, 16, 10) == 45535 + 12768
    assert centre(s, 16, 255, 32767) == 45535                           # T = 8 388 352: flat


# ---- the soft clip is worth running ----
@pytest.mark.parametrize("depth", DEPTHS, ids=lambda d: "bits%d" % d[0])
@pytest.mark.parametrize("size", SOFT_SIZES, ids=lambda s: "%dx%d" % s)
def test_the_soft_clip_meets_every_class(size, depth):
    s = R.clip(*size, depth, "soft")[0][0]
    sh = R.shares(s, depth[0])
    print(size, depth, sh)
    for name in (R.FLAT, R.SHARP, R.BLURRED, R.LEVELLED):
        assert sh[name] >= 0.01, (name, sh)
    assert sh["vertical"] >= 0.10 and sh["repaired"] >= 0.05, sh


# ---- the interface ----
PROTOTYPE = ("int amtgpu_edgelevel(AmtGpuContext* ctx, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int width, int height, int nframes, "
             "int strength, int threshold, int repair);")


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_binding_and_library_carry_the_entry_point():
    from amatsukaze_amd import build as b
    b.build()
    import amatsukaze_amd as pkg
    raw = open(os.path.join(ROOT, "include", "amt_gpu.h")).read()
    assert squeeze(PROTOTYPE) in squeeze(raw)
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", raw, re.M)                        # an addition only
    from amatsukaze_amd import binding
    c_i, c_p = C.c_int, C.c_void_p
    assert binding.SIGNATURES["amtgpu_edgelevel"] == (c_i, [c_p, c_p, c_p] + [c_i] * 6)
    assert "edge_level" in pkg.__all__ and callable(pkg.edge_level)
    assert {"amt_gpu_edgelevel.hip", "edgelevel_kernels.hip"} <= set(b.SOURCES)
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    assert "amtgpu_edgelevel" in set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    assert binding.load().amtgpu_abi_version() == 5


def test_the_launcher_is_declared_once_and_defined_once():
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f))}
    decl = [f for f, t in files.items() if re.search(r"hipError_t\s+launch_edgelevel\s*\([^)]*\)\s*;", t)]
    defs = [f for f, t in files.items() if re.search(r"hipError_t\s+launch_edgelevel\s*\([^)]*\)\s*\{", t)]
    assert decl == ["kernels.hpp"] and defs == ["edgelevel_kernels.hip"], (decl, defs)
    assert [f for f, t in files.items() if re.search(r"\bstruct EdgeLevelArgs\b", t)] == ["kernels.hpp"]
    assert [f for f, t in files.items() if re.search(r"\bedgelevel_vec16\(", t)] == ["amt_gpu_edgelevel.hip", "lane_rule.h"]
    assert [f for f, t in files.items() if re.search(r"\bkEdgeLevelPair\b", t)] == ["amt_gpu_edgelevel.hip", "plane_pair.hpp"]
    assert '#include "edgelevel_body.h"' in files["edgelevel_kernels.hip"] and "edge_pixel" in files["edgelevel_body.h"]
    assert 'prof_begin("edgelevel_kernel")' in files["amt_gpu_edgelevel.hip"]
    for f in ("amt_gpu_edgelevel.hip", "edgelevel_kernels.hip"):
        assert re.search(r'^#include\s+[<"]([^>"]+)[>"]', files[f], re.M).group(1) == "build_knobs.h", f
    # the constants the GPU and ISA tests mirror
    assert re.search(r"^constexpr int kEdgeStripRows = 32;$", files["kernels.hpp"], re.M)
    assert re.search(r"^constexpr int kEdgeSpanBytes = 64 \* 16;$", files["kernels.hpp"], re.M)
    import test_gpu_edgelevel as G
    assert (G.STRIP, G.SPAN_BYTES) == (32, 64 * 16)


def test_the_lane_rule_takes_every_operand(tmp_path):
    """edgelevel_vec16 against the definition: 16 divides every base, stride and pitch of all four plane kinds, and the row lengths"""
    out = str(tmp_path / "edgelevel_lane_rule_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(CPP, "edgelevel_lane_rule_test.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no difference" in r.stdout
