"""CPU side of the cadence renderer's edge-directed, motion-adaptive bob: the numpy restatement
(tests/kfm_render_adaptive_ref.py) on the literal diagonal known answer, the range property at 8, 10 and 16 bits with planted extremes,
a clip cut into batches with one-frame halos, and the new entry point in the header, the binding and the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kfm_render_adaptive_ref as A
import kfm_render_ref as R
from amtlib import ROOT

W_, T_, B_ = R.WEAVE, R.BOB_TOP, R.BOB_BOTTOM
PROTOTYPE = ("int amtgpu_kfm_render_deint(AmtGpuContext* ctx, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height, "
             "const AmtGpuRenderFrame* plan, int nout, int deint, int thresh, const AmtGpuSurfaces* dst);")
CSRC = os.path.join(ROOT, "amatsukaze_amd", "csrc")


@pytest.fixture(scope="module")
def pkg():
    from amatsukaze_amd import build as b
    b.build()
    import amatsukaze_amd
    return amatsukaze_amd


def diagonal_clip():
    """three frames of 16x8 luma: frame 1 has row y at 0 left of column 4 + y and at 200 from there, frame 0 is all 0, frame 2 all 255"""
    Y = np.zeros((3, 8, 16), np.uint8)
    Y[2] = 255
    for y in range(8):
        Y[1, y] = np.where(np.arange(16) < 4 + y, 0, 200)
    UV = np.zeros((3, 4, 8), np.uint8)
    return Y, UV, UV.copy()


def test_the_diagonal_known_answer():
    planes = diagonal_clip()
    (Y, _, _), counts = A.render_adaptive_ref(planes, [(T_, 1, 1, 1), (B_, 1, 1, 1)])
    assert list(Y[0, 3]) == [0] * 7 + [200] * 9                                              # the exact diagonal: 0 for x < 7, 200 from x = 7
    assert list(Y[1, 4]) == [0] * 8 + [200] * 8
    for y in range(0, 8, 2):
        assert np.array_equal(Y[0, y], planes[0][1, y])                                      # kept rows
    line = R.render_ref(planes, [(T_, 1, 1, 1)], -1)[0]
    assert list(line[0, 3]) == [0] * 6 + [100, 100] + [200] * 8                              # the line rule's staircase at columns 6 and 7
    assert sum(counts[0]["dir"]) == sum(counts[0]["clamp"]) == 2 * 4 * 16


def planted_clip(bits, shape, seed):
    """random containers over the depth's range with 0 and the largest container planted in one frame and its neighbour"""
    n, h, w = shape
    rng = np.random.default_rng(seed)
    dt = np.uint8 if bits == 8 else np.uint16
    top = 255 if bits == 8 else 65535
    planes = []
    for hh, ww in ((h, w), (h // 2, w // 2), (h // 2, w // 2)):
        P = rng.integers(0, 1 << bits, (n, hh, ww)).astype(dt)
        P[1, hh // 2 - 1:hh // 2 + 2, 1:ww - 1:3] = top
        P[1, hh // 2 - 1:hh // 2 + 2, 2:ww - 1:3] = 0
        P[2, hh // 2 - 2:hh // 2 + 3, 1:ww - 1:2] = 0
        P[2, hh // 2 - 2:hh // 2 + 3, 2:ww - 1:2] = top
        P[0, 0, 0] = P[n - 1, hh - 1, ww - 1] = top
        planes.append(P)
    return tuple(planes), top


@pytest.mark.parametrize("bits, shape", [(8, (4, 18, 44)), (10, (4, 18, 45 * 2)), (16, (4, 18, 44))])
def test_the_output_stays_in_the_containers_range(bits, shape):
    planes, top = planted_clip(bits, shape, 100 + bits)
    n = shape[0]
    plan = [e for k in range(n) for e in ((T_, k, k, 1), (B_, k, k, 1))]
    out, counts = A.render_adaptive_ref(planes, plan)                                        # (asserts the range row by row before it narrows)
    for k in range(3):
        assert out[k].dtype == planes[k].dtype and out[k].shape == (2 * n,) + planes[k].shape[1:]
        assert int(out[k].max()) <= top and all(c > 0 for c in counts[k]["dir"]) and all(c > 0 for c in counts[k]["clamp"])
        # kept rows are the source's
        assert np.array_equal(out[k][0::2, 0::2], planes[k][:, 0::2]) and np.array_equal(out[k][1::2, 1::2], planes[k][:, 1::2])
    if bits == 10:
        assert int(max(p.max() for p in planes)) == 65535                                    # containers beyond 10 bits are taken as stored


def test_the_smallest_plane_is_well_defined():
    planes = tuple(np.array([[[7], [200]], [[90], [3]], [[255], [0]]], np.uint8) for _ in range(3))       # 1 wide, 2 high, 3 frames
    out, _ = A.render_adaptive_ref(planes, [(T_, 1, 1, 1), (B_, 1, 1, 1)])
    assert out[0].shape == (2, 2, 1) and out[0][0, 0, 0] == 90 and out[0][1, 1, 0] == 3


def test_random_small_planes_take_every_direction_and_clamp():
    rng = np.random.default_rng(3)
    planes = tuple(rng.integers(0, 256, (3, 6, 11)).astype(np.uint8) for _ in range(3))
    _, counts = A.render_adaptive_ref(planes, [(T_, k, k, 1) for k in range(3)] + [(B_, k, k, 1) for k in range(3)])
    assert sum(counts[0]["dir"]) == 198 and all(c > 0 for c in counts[0]["dir"]) and all(c > 0 for c in counts[0]["clamp"])


def test_batches_with_one_frame_halos_give_the_frames_of_one_call():
    rng = np.random.default_rng(9)
    N = 6
    planes = tuple(rng.integers(0, 256, (N, h, w)).astype(np.uint8) for h, w in ((12, 22), (6, 11), (6, 11)))
    plan = R.plan_array([e for n in range(N) for e in ((T_, n, n, 1), (B_, n, n, 1))] + [(W_, 3, 2, 2)])
    whole, _ = A.render_adaptive_ref(planes, plan)
    for lo, hi in ((0, 2), (2, 4), (4, 6)):
        a, b = max(0, lo - 1), min(N, hi + 1)
        own = [i for i, e in enumerate(plan) if lo <= e["top"] < hi]
        part, _ = A.render_adaptive_ref(tuple(p[a:b] for p in planes), plan[own], clip_first=a, clip_frames=N)
        for k in range(3):
            assert np.array_equal(part[k], whole[k][own]), (lo, hi, k)
    # without the halo the bytes differ: the batch is not the clip
    alone, _ = A.render_adaptive_ref(tuple(p[2:4] for p in planes), plan[0:4])            # frames 2 and 3 as a clip of their own
    assert not np.array_equal(alone[0], whole[0][4:8])


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_binding_and_library_carry_the_entry_point(pkg):
    raw = open(os.path.join(ROOT, "include", "amt_gpu.h")).read()
    assert squeeze(PROTOTYPE) in squeeze(raw)
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", raw, re.M)                        # additions only
    for name, value in (("LINE", 0), ("ADAPTIVE", 1)):
        assert re.search(rf"^#define AMTGPU_DEINT_{name}\s+{value}\b", raw, re.M), name
    from amatsukaze_amd import api, binding, build as b
    c_i, c_p = C.c_int, C.c_void_p
    assert binding.SIGNATURES["amtgpu_kfm_render_deint"] == (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_i, c_i, c_i, c_p])
    assert binding.SIGNATURES["amtgpu_kfm_render"] == (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_i, c_i, c_p])      # as it was
    assert (api.DEINT_LINE, api.DEINT_ADAPTIVE) == (0, 1) == (pkg.DEINT_LINE, pkg.DEINT_ADAPTIVE)
    assert {"DEINT_LINE", "DEINT_ADAPTIVE", "kfm_render"} <= set(pkg.__all__)
    assert "render_adaptive_kernels.hip" in b.SOURCES
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    assert {"amtgpu_kfm_render_deint", "amtgpu_kfm_render"} <= set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    assert binding.load().amtgpu_abi_version() == 5


def test_the_launcher_is_declared_once_and_defined_once():
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC))}
    decl = [f for f, t in files.items() if re.search(r"hipError_t\s+launch_kfm_render_adaptive\s*\([^)]*\)\s*;", t)]
    defs = [f for f, t in files.items() if re.search(r"hipError_t\s+launch_kfm_render_adaptive\s*\([^)]*\)\s*\{", t)]
    assert decl == ["kernels.hpp"] and defs == ["render_adaptive_kernels.hip"]
    assert [f for f, t in files.items() if re.search(r"struct\s+RenderAdaptiveEntry\s*\{", t)] == ["kernels.hpp"]


def test_the_line_rules_helpers_stay_in_render_body_alone():
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC))}
    for name in ("render_avg", "render_within", "render_mix", "render_fill_row"):
        defs = [f for f, t in files.items() if re.search(rf"\b(uint32_t|void)\s+{name}\s*\(", t)]
        assert defs == ["render_body.h"], (name, defs)
    assert not re.search(r"\brender_(avg|within|mix|fill_row)\b", files["render_adaptive_kernels.hip"])


def test_python_refuses_an_unknown_rule_before_any_call(pkg):
    with pytest.raises(pkg.AmtError, match="deint"):
        pkg.kfm_render(None, None, [], None, deint="yadif")
