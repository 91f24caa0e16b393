"""CPU side of the cadence renderer on decoder surfaces: the numpy restatement (tests/kfm_render_surfaces_ref.py) against the planar one
(kfm_render_ref.render_ref) on the planarised samples -- the identity of DESIGN.md section 6d on random clips with random non-zero low
bits -- and the new kernel file's place in the build, the launcher's one declaration and the unchanged ABI."""
import os
import re

import numpy as np
import pytest

import kfm_render_ref as R
import kfm_render_surfaces_ref as S
from amtlib import ROOT

W_, T_, B_ = R.WEAVE, R.BOB_TOP, R.BOB_BOTTOM
PLAN = R.plan_array([(W_, 0, 0, 2), (W_, 3, 2, 2), (W_, 2, 3, 2), (T_, 0, 0, 1), (B_, 5, 5, 1), (T_, 4, 4, 1), (B_, 4, 4, 1), (T_, 5, 5, 1), (B_, 0, 0, 1)])

# (bits, interleaved, msb)
KINDS = {"nv12": (8, True, False), "p010": (10, True, True), "p012": (12, True, True), "p016": (16, True, True), "interleaved-lsb-10": (10, True, False),
         "planar-msb-10": (10, False, True), "planar-msb-9": (9, False, True)}


def random_surface(rng, n, w, h, bits, interleaved, msb):
    """tight container planes with every bit of the container random (the low bits of MSB-aligned ones included)"""
    dt, top = (np.uint8, 256) if bits <= 8 else (np.uint16, 1 << 16 if msb else 1 << bits)
    mk = lambda rows, cols: rng.integers(0, top, (n, rows, cols)).astype(dt)
    return (mk(h, w), mk(h // 2, w)) if interleaved else (mk(h, w), mk(h // 2, w // 2), mk(h // 2, w // 2))


@pytest.mark.parametrize("thresh", (-1, 0, 3, 40, 65535))
@pytest.mark.parametrize("kind", list(KINDS))
def test_the_restatement_is_the_planar_rule_on_the_samples(kind, thresh):
    bits, interleaved, msb = KINDS[kind]
    rng = np.random.default_rng(sum(map(ord, kind)) + 11)
    w, h, n = 14, 10, 6
    src = random_surface(rng, n, w, h, bits, interleaved, msb)
    s = S.shift_of(bits, msb)
    low = (1 << s) - 1
    if s:
        assert all((p & low).any() for p in src)                                      # the low bits are not zero
    got = S.split_planes(S.render_surfaces_ref(src, PLAN, thresh, bits, interleaved, msb), interleaved)
    planar = S.split_planes(src, interleaved)
    t = thresh if not s or thresh < 0 else min(thresh, (1 << bits) - 1)
    want = R.render_ref(tuple(p >> s for p in planar), PLAN, t)
    for g, e, p in zip(got, want, planar):
        assert g.dtype == p.dtype and np.array_equal(g >> s, e)                       # dst >> s is the planar LSB render of src >> s
        for k, entry in enumerate(PLAN):
            for parity, frame in S.copied_rows(entry, 0):
                assert np.array_equal(g[k, parity::2], p[frame, parity::2])           # copied rows are their source rows, low bits included
            ip = S.interpolated_rows(entry)
            if ip is not None:
                assert not (g[k, ip::2] & low).any()                                  # interpolated containers have zero low bits
    if s == 0:
        for g, e in zip(got, R.render_ref(planar, PLAN, thresh)):
            assert np.array_equal(g, e)                                               # LSB: containers as stored, no masking to bits


def test_a_batch_with_its_halo_gives_the_rows_of_the_whole_clip():
    bits, interleaved, msb = KINDS["p010"]
    src = random_surface(np.random.default_rng(3), 6, 14, 10, bits, interleaved, msb)
    whole = S.render_surfaces_ref(src, PLAN, 3, bits, interleaved, msb)
    own = [i for i, e in enumerate(PLAN) if 2 <= e["top"] < 5 and 2 <= e["bottom"] < 5]
    part = S.render_surfaces_ref(tuple(p[1:6] for p in src), PLAN[own], 3, bits, interleaved, msb, clip_first=1, clip_frames=6)
    for a, b in zip(whole, part):
        assert np.array_equal(a[own], b)


def test_the_kernel_file_is_built_and_its_launcher_declared_once():
    from amatsukaze_amd import build as b
    assert "render_surface_kernels.hip" in b.SOURCES and "render_kernels.hip" in b.SOURCES
    csrc = os.path.join(ROOT, "amatsukaze_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if os.path.isfile(os.path.join(csrc, f))}
    decl = [f for f, t in text.items() if re.search(r"hipError_t\s+launch_kfm_render_surfaces\s*\([^)]*\)\s*;", t)]
    assert decl == ["kernels.hpp"]
    defs = [f for f, t in text.items() if re.search(r"hipError_t\s+launch_kfm_render_surfaces\s*\([^)]*\)\s*\{", t)]
    assert defs == ["render_surface_kernels.hip"]
    assert "launch_kfm_render_surfaces(" in text["amt_gpu_render.hip"] and "launch_kfm_render(" in text["amt_gpu_render.hip"]
    # one text of the packed helpers for both kernel files
    for helper in ("render_avg", "render_within", "render_mix", "render_fill_row"):
        assert [f for f, t in text.items() if re.search(rf"uint32_t {helper}\(|void {helper}\(", t)] == ["render_body.h"], helper
    raw = open(os.path.join(ROOT, "include", "amt_gpu.h")).read()
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", raw, re.M)                    # no new entry point, no new signature
    b.build()
    from amatsukaze_amd import binding
    assert binding.load().amtgpu_abi_version() == 5
