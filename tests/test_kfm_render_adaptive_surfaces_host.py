"""CPU side of the adaptive bob on decoder surfaces ("the adaptive rule on surfaces"): the composed numpy
restatement (tests/kfm_render_adaptive_surfaces_ref.py) on a literal diagonal known answer IN CHROMA, the proof that walking an
interleaved UV plane as one plane of `width` containers (the line kernel's trick) is wrong under this rule, the MSB and depth properties,
a clip cut into batches with one-frame halos, and the new entry point in the header, the binding, the build and the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kfm_render_adaptive_ref as A
import kfm_render_adaptive_surfaces_ref as AS
import kfm_render_ref as R
import kfm_render_surfaces_ref as S
from amtlib import ROOT

W_, T_, B_ = R.WEAVE, R.BOB_TOP, R.BOB_BOTTOM
PROTOTYPE = ("int amtgpu_kfm_render_deint_surfaces(AmtGpuContext* ctx, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, "
             "int height, const AmtGpuRenderFrame* plan, int nout, int deint, int thresh, const AmtGpuSurfaces* dst);")
CSRC = os.path.join(ROOT, "amatsukaze_amd", "csrc")
# the plan of tests/test_gpu_kfm_render_adaptive.py: both bobs at frame 0, mid-clip and at the last frame, three weaves, six source frames
PLAN = R.plan_array([(T_, 0, 0, 1), (B_, 0, 0, 1), (W_, 3, 2, 2), (T_, 2, 2, 1), (B_, 2, 2, 1), (W_, 1, 1, 2), (W_, 2, 3, 2), (T_, 5, 5, 1), (B_, 5, 5, 1),
                     (T_, 3, 3, 1), (B_, 3, 3, 1)])
NSRC = 6


@pytest.fixture(scope="module")
def pkg():
    from amatsukaze_amd import build as b
    b.build()
    import amatsukaze_amd
    return amatsukaze_amd


def random_planes(rng, n, w, h, bits, interleaved, msb):
    """tight container planes of a clip: MSB-aligned ones with random low bits"""
    dt = np.uint8 if bits <= 8 else np.uint16
    top = 256 if bits <= 8 else 1 << 16 if msb else 1 << bits
    shapes = [(n, h, w), (n, h // 2, w)] if interleaved else [(n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2)]
    return tuple(rng.integers(0, top, sh).astype(dt) for sh in shapes)


def test_the_diagonal_known_answer_in_chroma():
    n, w, h, x0 = 3, 64, 16, 5
    rng = np.random.default_rng(1)
    Y = rng.integers(0, 256, (n, h, w)).astype(np.uint8)
    U = np.zeros((n, h // 2, w // 2), np.uint8)
    U[2] = 255
    for y in range(8):
        U[1, y, x0:x0 + 16] = np.where(np.arange(16) < 4 + y, 0, 200)
    V = np.broadcast_to(((np.arange(w // 2) * 37 + 11) % 256).astype(np.uint8), U.shape).copy()          # static, and unlike U
    (_, UV) = S.join_planes((Y, U, V), True)
    (Yo, UVo), counts = AS.render_adaptive_surfaces_ref((Y, UV), [(T_, 1, 1, 1), (B_, 1, 1, 1)], 8, True, False)
    Uo, Vo = UVo[:, :, 0::2], UVo[:, :, 1::2]
    assert list(Uo[0, 3, x0 + 3:x0 + 13]) == [0] * 4 + [200] * 6
    assert list(Uo[1, 4, x0 + 3:x0 + 13]) == [0] * 5 + [200] * 5
    assert np.array_equal(Vo[0], V[1]) and np.array_equal(Vo[1], V[1])
    assert np.array_equal(UVo[0, 0::2], UV[1, 0::2]) and np.array_equal(UVo[1, 1::2], UV[1, 1::2])       # kept rows
    assert sum(counts[1]["dir"]) == sum(counts[2]["clamp"]) == 2 * 4 * 32


@pytest.mark.parametrize("bits, msb", [(8, False), (10, True)])
def test_walking_the_uv_plane_as_one_plane_is_wrong(bits, msb):
    w, h = 96, 36
    planes = random_planes(np.random.default_rng(20 + bits), NSRC, w, h, bits, True, msb)
    want, _ = AS.render_adaptive_surfaces_ref(planes, PLAN, bits, True, msb)
    short = AS.shortcut_ref(planes, PLAN, bits, msb)
    assert np.array_equal(want[0], short[0])                                                 # luma is one plane either way
    total = differ = 0
    for k, e in enumerate(PLAN):
        ip = S.interpolated_rows(e)
        if ip is None:
            assert np.array_equal(want[1][k], short[1][k])
            continue
        assert np.array_equal(want[1][k, 1 - ip::2], short[1][k, 1 - ip::2])                 # copied rows are copied either way
        total += want[1][k, ip::2].size
        differ += int((want[1][k, ip::2] != short[1][k, ip::2]).sum())
    print("interpolated UV containers that differ:", differ, "of", total)
    assert total == 6912 and differ > total // 4


@pytest.mark.parametrize("name, bits, interleaved, msb", [("p010", 10, True, True), ("p012", 12, True, True), ("planar-msb-10", 10, False, True),
                                                          ("interleaved-lsb-10", 10, True, False), ("p016", 16, True, True)])
def test_msb_and_depth_properties(name, bits, interleaved, msb):
    w, h = 34, 12
    s = S.shift_of(bits, msb)
    planes = random_planes(np.random.default_rng(bits * 7 + interleaved), NSRC, w, h, bits, interleaved, msb)
    if s:
        assert any((p & ((1 << s) - 1)).any() for p in planes)                                # random low bits in the source
    got, _ = AS.render_adaptive_surfaces_ref(planes, PLAN, bits, interleaved, msb)
    low = (1 << s) - 1
    for k, e in enumerate(PLAN):
        ip = S.interpolated_rows(e)
        for g, p in zip(got, planes):
            for parity, frame in S.copied_rows(e, 0):
                assert np.array_equal(g[k, parity::2], p[frame, parity::2])
            if ip is not None:
                assert not (g[k, ip::2] & low).any()
    planar, _ = A.render_adaptive_ref(tuple(np.ascontiguousarray(p >> s) for p in S.split_planes(planes, interleaved)), PLAN)
    for g, p in zip(S.split_planes(got, interleaved), planar):
        assert np.array_equal(g >> s, p)
    if not s:
        # containers as stored: nothing is shifted, so the surfaces' render IS the planar render re-interleaved
        for g, p in zip(got, S.join_planes(planar, interleaved)):
            assert np.array_equal(g, p)


@pytest.mark.parametrize("bits, msb", [(8, False), (10, True)])
def test_batches_with_one_frame_halos_give_the_frames_of_one_call(bits, msb):
    N = 6
    planes = random_planes(np.random.default_rng(9 + bits), N, 22, 12, bits, True, msb)
    plan = R.plan_array([e for n in range(N) for e in ((T_, n, n, 1), (B_, n, n, 1))] + [(W_, 3, 2, 2)])
    whole, _ = AS.render_adaptive_surfaces_ref(planes, plan, bits, True, msb)
    for lo, hi in ((0, 2), (2, 4), (4, 6)):
        a, b = max(0, lo - 1), min(N, hi + 1)
        own = [i for i, e in enumerate(plan) if lo <= e["top"] < hi]
        part, _ = AS.render_adaptive_surfaces_ref(tuple(p[a:b] for p in planes), plan[own], bits, True, msb, clip_first=a, clip_frames=N)
        for k in range(2):
            assert np.array_equal(part[k], whole[k][own]), (lo, hi, k)


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_binding_and_library_carry_the_entry_point(pkg):
    raw = open(os.path.join(ROOT, "include", "amt_gpu.h")).read()
    assert squeeze(PROTOTYPE) in squeeze(raw)
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", raw, re.M)                        # an addition only
    assert "not built yet" not in raw
    from amatsukaze_amd import binding, build as b
    c_i, c_p = C.c_int, C.c_void_p
    assert binding.SIGNATURES["amtgpu_kfm_render_deint_surfaces"] == (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_i, c_i, c_i, c_p])
    assert binding.SIGNATURES["amtgpu_kfm_render_deint_surfaces"] == binding.SIGNATURES["amtgpu_kfm_render_deint"]          # argument for argument
    assert "render_adaptive_surface_kernels.hip" in b.SOURCES and "render_adaptive_kernels.hip" in b.SOURCES
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    assert {"amtgpu_kfm_render_deint_surfaces", "amtgpu_kfm_render_deint", "amtgpu_kfm_render"} <= set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    assert binding.load().amtgpu_abi_version() == 5


def test_the_launcher_is_declared_once_and_defined_once():
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC))}
    decl = [f for f, t in files.items() if re.search(r"hipError_t\s+launch_kfm_render_adaptive_surfaces\s*\([^)]*\)\s*;", t)]
    defs = [f for f, t in files.items() if re.search(r"hipError_t\s+launch_kfm_render_adaptive_surfaces\s*\([^)]*\)\s*\{", t)]
    assert decl == ["kernels.hpp"] and defs == ["render_adaptive_surface_kernels.hip"]
    # the rule's text is shared, not pasted: one definition, in the header both kernel files include
    for name in ("adp_pixel", "adp_fill_row", "adp_one", "adp_ld"):
        assert [f for f, t in files.items() if re.search(rf"\b{name}\s*\([^;{{]*\)\s*\{{", t)] == ["render_adaptive_body.h"], name
    for f in ("render_adaptive_kernels.hip", "render_adaptive_surface_kernels.hip"):
        assert '#include "render_adaptive_body.h"' in files[f], f
