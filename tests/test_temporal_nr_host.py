"""CPU side of the temporal noise reduction (amtgpu_temporal_nr): the numpy restatement
(tests/temporal_nr_ref.py) against what the reference's own TemporalNRFilter wrote (tests/golden/temporal_nr_v1.npz, made by
tools/make_temporal_nr_golden.py), the replay of its onFrame / finish stream against the clamp rule, the entry point in the header, the
binding and the library, and the lane rule against a brute-force check."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import temporal_nr_ref as R
from amtlib import ROOT

PROTOTYPE = ("int amtgpu_temporal_nr(AmtGpuContext* ctx, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height, "
             "int out_first, int nout, int temporal_distance, int threshold, int interlaced, const AmtGpuSurfaces* dst);")
CSRC = os.path.join(ROOT, "amatsukaze_amd", "csrc")
NCASES = 6


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "temporal_nr_v1.npz"))


def test_the_golden_covers_what_it_is_meant_to(golden):
    params = [tuple(int(v) for v in golden[f"c{k}_params"]) for k in range(NCASES)]
    assert {p[0] for p in params} == {8, 10, 14, 16} and {p[1] for p in params} == {0, 1, 3} and {p[3] for p in params} == {0, 1}
    assert any(golden[f"c{k}_Y"].shape[0] == 2 * params[k][1] > 0 for k in range(NCASES))              # a clip of exactly 2 d frames
    assert int(golden["c1_Y"].max()) > 1023                                                              # a container above maxv at 10 bits


@pytest.mark.parametrize("k", range(NCASES))
def test_the_restatement_equals_the_compiled_reference(golden, k):
    bits, d, thr, il = (int(v) for v in golden[f"c{k}_params"])
    planes = tuple(golden[f"c{k}_{p}"] for p in "YUV")
    n = planes[0].shape[0]
    assert list(golden[f"c{k}_idx"]) == list(range(n))                     # n >= 2 d: the reference emits every frame, in order
    Y, U, V, count = R.filter_clip(planes, d, thr, bits, bool(il))
    for name, got in (("oY", Y), ("oU", U), ("oV", V)):
        want = golden[f"c{k}_{name}"]
        assert got.dtype == want.dtype and np.array_equal(got, want), (k, name, int(np.sum(got != want)))
    if d:
        assert len(np.unique(count)) > 1 and not np.array_equal(Y, planes[0])          # the filter did something


@pytest.mark.parametrize("d", range(6))
def test_the_reference_stream_is_the_clamp_rule_from_2d_frames_on(d):
    for n in range(max(2 * d, 1), 2 * d + 10):
        assert R.stream_windows(d, n) == [(t, R.window(t, d, n)) for t in range(n)], (d, n)


def test_the_replay_drops_the_frames_the_reference_drops(golden):
    assert [c for c, _ in R.stream_windows(3, 5)] == list(golden["short5_idx"]) == [0, 1, 3, 4]
    assert [c for c, _ in R.stream_windows(3, 3)] == list(golden["short3_idx"]) == []
    # (frame 2 of the 5 never comes out; amtgpu_temporal_nr keeps the clamp rule for every length and emits all of them)


def test_the_wrong_variants_differ_only_in_rounding():
    rng = np.random.default_rng(4)
    planes = R.make_clip(12, 34, 8, 8, 1, rng)
    ref = R.filter_clip(planes, 3, 1, 8)
    for v in ("fma", "reversed", "rational"):
        got = R.filter_clip(planes, 3, 1, 8, variant=v)
        for k in range(3):
            assert np.abs(got[k].astype(int) - ref[k].astype(int)).max() <= 1, v
        assert np.array_equal(got[3], ref[3])


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_binding_and_library_carry_the_entry_point():
    from amatsukaze_amd import build as b
    b.build()
    import amatsukaze_amd as pkg
    raw = open(os.path.join(ROOT, "include", "amt_gpu.h")).read()
    assert squeeze(PROTOTYPE) in squeeze(raw)
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", raw, re.M)                        # an addition
    from amatsukaze_amd import binding
    c_i, c_p = C.c_int, C.c_void_p
    assert binding.SIGNATURES["amtgpu_temporal_nr"] == (c_i, [c_p, c_p] + [c_i] * 10 + [c_p])
    assert "temporal_nr" in pkg.__all__ and callable(pkg.temporal_nr)
    assert {"temporal_nr_kernels.hip", "amt_gpu_tnr.hip"} <= set(b.SOURCES)
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    assert "amtgpu_temporal_nr" in set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    assert binding.load().amtgpu_abi_version() == 5


def test_the_launcher_is_declared_once_and_defined_once():
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f))}
    decl = [f for f, t in files.items() if re.search(r"hipError_t\s+launch_temporal_nr\s*\([^)]*\)\s*;", t)]
    defs = [f for f, t in files.items() if re.search(r"hipError_t\s+launch_temporal_nr\s*\([^)]*\)\s*\{", t)]
    assert decl == ["kernels.hpp"] and defs == ["temporal_nr_kernels.hip"]
    assert [f for f, t in files.items() if re.search(r"\btemporal_nr_vec16\(", t)] == ["amt_gpu_tnr.hip", "lane_rule.h"]


def test_the_lane_rule_against_brute_force(tmp_path):
    out = str(tmp_path / "temporal_nr_lane_rule_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "temporal_nr_lane_rule_test.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no difference" in r.stdout
