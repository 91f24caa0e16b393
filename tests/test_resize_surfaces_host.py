"""CPU side of the resize on decoder surfaces (amtgpu_resize_run_surfaces; DESIGN.md section 6e, "surfaces in kind"): the entry point in
the header, the binding and the library; the new launchers declared once and defined once; the lane rule against brute force and the
pair run-length rule's numpy port against the C++ one (both through tests/cpp/resize_surface_rules_test.cpp, built with g++); that every
read of a zero tap behind a staged span lands inside the wave's region; and the composed restatement against itself on what the rule
promises (low bits, equal sizes, the planar route on the same samples)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import resize_ref as R
import resize_surfaces_ref as RS
import temporal_nr_surfaces_ref as TS
from amtlib import ROOT
from test_resize_host import squeeze

CSRC = os.path.join(ROOT, "amatsukaze_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")

PROTOTYPE = "int amtgpu_resize_run_surfaces(AmtGpuResize* r, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes);"


@pytest.fixture(scope="module")
def rules_test(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("resize_surfaces") / "resize_surface_rules_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(CPP, "resize_surface_rules_test.cpp"),
                           os.path.join(CSRC, "resize_plan.cpp"), "-o", out])
    return out


def test_header_binding_and_library_carry_the_entry_point():
    from amatsukaze_amd import build as b
    b.build()
    raw = open(os.path.join(ROOT, "include", "amt_gpu.h")).read()
    assert squeeze(PROTOTYPE) in squeeze(raw)
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", raw, re.M)                        # an addition
    from amatsukaze_amd import binding
    c_i, c_p = C.c_int, C.c_void_p
    assert binding.SIGNATURES["amtgpu_resize_run_surfaces"] == (c_i, [c_p, c_p, c_p, c_i]) == binding.SIGNATURES["amtgpu_resize_run"]
    assert {"resize_kernels.hip", "resize_surface_kernels.hip"} <= set(b.SOURCES)
    assert b.SOURCES.index("resize_surface_kernels.hip") == b.SOURCES.index("resize_kernels.hip") + 1
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    assert {"amtgpu_resize_run", "amtgpu_resize_run_surfaces"} <= set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    assert binding.load().amtgpu_abi_version() == 5


def test_the_launchers_are_declared_once_and_defined_once():
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f))}
    for name in ("launch_resize_surfaces_h", "launch_resize_surfaces_v"):
        decl = [f for f, t in files.items() if re.search(rf"hipError_t\s+{name}\s*\([^)]*\)\s*;", t)]
        defs = [f for f, t in files.items() if re.search(rf"hipError_t\s+{name}\s*\([^)]*\)\s*\{{", t)]
        assert decl == ["kernels.hpp"] and defs == ["resize_surface_kernels.hip"], (name, decl, defs)
    assert [f for f, t in files.items() if re.search(r"\bresize_surface_vec16\(", t)] == ["amt_gpu_resize.hip", "lane_rule.h"]
    assert [f for f, t in files.items() if re.search(r"\bresize_pair_columns_per_wave\(", t)] == ["amt_gpu_resize.hip", "resize_plan.cpp", "resize_region.h"]
    # the kernel sizes its LDS and the host refuses by the same constants
    region = files["resize_region.h"]
    assert int(re.search(r"kResizeRegionBytes = (\d+);", region).group(1)) == RS.REGION_BYTES
    assert int(re.search(r"kResizePairSlack = (\d+);", region).group(1)) == RS.PAIR_SLACK
    assert int(re.search(r"kResizeMaxZeroTaps = (\d+);", region).group(1)) == RS.MAX_ZERO_TAPS
    assert "kResizeRegionBytes" in files["resize_surface_kernels.hip"] and "kResizePairSlack" in files["amt_gpu_resize.hip"]


def test_the_rounding_the_item_rule_and_the_vertical_cell_are_defined_once():
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f))}
    for name in ("resize_mad", "resize_round", "resize_item", "resize_load", "resize_store", "resize_v_cell", "resize_args_ok"):
        defs = [f for f, t in files.items() if re.search(rf"\b(?:int|void|bool|ResizeItem)\s+{name}\s*\(", t)]       # (a return type in front: no call)
        assert defs == ["resize_body.h"], (name, defs)
    # the rounding's constants appear where it is defined and nowhere else
    assert [f for f, t in files.items() if re.search(r"\+\s*8192\s*\)\s*>>\s*14", re.sub(r"//.*", "", t))] == ["resize_body.h"]
    both = ("resize_kernels.hip", "resize_surface_kernels.hip")
    assert [f for f, t in files.items() if re.search(r'^#include "resize_body\.h"', t, re.M)] == list(both)
    for f in both:
        assert all(re.search(rf"\b{name}\s*[<(]", files[f]) for name in ("resize_round", "resize_item", "resize_v_cell", "resize_grid")), f
    assert re.search(r"^#pragma once", files["resize_body.h"], re.M) and not re.search(r"^\s*__global__", files["resize_body.h"], re.M)
    left = [(f, m) for f, t in files.items() for m in re.findall(r"\bresize_surface_(?:mad|round|item|load|store|v_cell)\b|\bResizeSurfaceItem\b", t)]
    assert not left, left


def test_the_lane_rule_against_brute_force(rules_test):
    r = subprocess.run([rules_test], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no difference" in r.stdout


# chroma axes (S, D) in pairs: those of the GPU tests, and S = 4 D .. 80 D for D = 8, 34, 64 -- from where a run of 32 pairs fits to where
# not one pair does
SWEEP = [(24, 16), (136, 91), (16, 25), (8, 4), (4, 2), (80, 16), (32, 32), (500, 8), (501, 8), (800, 8), (1248, 96), (176, 117), (960, 640)]
SWEEP += [(S, D) for D in (8, 34, 64) for S in range(4 * D, 80 * D + 1, 2 if D == 8 else 6)]


def test_the_pair_run_length_port_is_the_cpp_rule(rules_test):
    cases = [(S, D, "blackman", 0) for S, D in SWEEP]
    cases += [(S, D, k, 0) for S, D in ((1000, 33), (880, 33), (1024, 16), (136, 91)) for k in ("lanczos", "bilinear")]
    cases += [(S, D, "blackman", 8) for S, D in ((24, 16), (18, 12), (500, 33))]
    cases = [c + (es,) for c in cases for es in (1, 2)]
    args = [str(v) for S, D, k, taps, es in cases for v in (S, D, R.KERNELS[k], taps, es)]
    out = subprocess.run([rules_test, "pair"] + args, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases) >= 1000
    seen = set()
    for line, (S, D, k, taps, es) in zip(out, cases):
        cS, cD, ck, ctaps, ces, cK, ccpw = (int(v) for v in line.split())
        assert (cS, cD, ck, ctaps, ces) == (S, D, R.KERNELS[k], taps, es)
        cpw, K, spans = RS.pair_columns_per_wave(S, D, es, k, taps)
        assert (cpw, K) == (ccpw, cK), (S, D, k, taps, es, "port", cpw, K, "C++", ccpw, cK)
        assert (len(spans) == -(-D // cpw) and max(spans) + RS.PAIR_SLACK <= RS.REGION_BYTES) if cpw else spans == ()
        # a pair is twice a container: a pair run never takes more columns than the planar rule gives the same axis
        assert cpw <= R.columns_per_wave(S, D, es, k, taps)[0]
        seen.add(cpw)
    assert seen == {0, 1, 2, 4, 8, 16, 32}                            # the sweep meets every answer the rule has


def test_the_issues_sizes_follow_from_the_rule():
    # 16 bits, 16 output columns: chroma S / 2 -> 8 has K = S / 2 pairs, all windows at 0
    assert RS.pair_columns_per_wave(500, 8, 2) == (32, 500, (2000,)) and 2000 + RS.PAIR_SLACK == RS.REGION_BYTES
    assert RS.pair_columns_per_wave(501, 8, 2)[0] == 0 and R.columns_per_wave(501, 8, 2)[0] >= 1 and R.columns_per_wave(1002, 16, 2)[0] >= 1
    assert RS.pair_columns_per_wave(800, 8, 2)[0] == 0 and R.columns_per_wave(800, 8, 2)[0] >= 1 and R.columns_per_wave(1600, 16, 2)[0] >= 1
    # pair runs of 16 under luma runs of 64
    assert R.columns_per_wave(2496, 192, 2)[0] == 64 and RS.pair_columns_per_wave(1248, 96, 2)[0] == 16


def test_every_zero_tap_read_lands_inside_the_region():
    """A lane of a register form reads KR taps from its window's first container; those behind the K real ones carry a zero coefficient
    and may lie behind the staged span.  In the region the span begins up to 15 bytes in (it is staged from the 16 bytes it begins in),
    so the furthest byte a lane of column `col` reads is (start[col] + KR) * unit - (start[first] * unit & ~15), unit the bytes of a
    column: 2 * es in an interleaved row.  By the constants, for every K a register form takes; then on the programs of the sweep."""
    assert max(RS.register_taps(K) - K for K in range(1, 17)) == RS.MAX_ZERO_TAPS and all(RS.register_taps(K) >= K for K in range(1, 17))
    for es in (1, 2):
        for K in range(1, 17):
            assert RS.REGION_BYTES - RS.PAIR_SLACK + 15 + (RS.register_taps(K) - K) * 2 * es <= RS.REGION_BYTES, (K, es)
            assert R.REGION_BYTES - R.REGION_SLACK + 15 + (RS.register_taps(K) - K) * es <= R.REGION_BYTES, (K, es)
    met = set()
    for S, D in SWEEP:
        K, start = R.windows(S, D)
        KR = RS.register_taps(K)
        if not KR:
            continue
        for es in (1, 2):
            for unit, cpw in ((2 * es, RS.pair_columns_per_wave(S, D, es)[0]), (es, R.columns_per_wave(S, D, es)[0])):
                for c0 in range(0, D, cpw) if cpw else ():
                    last = min(c0 + cpw, D) - 1
                    furthest = (int(start[last]) + KR) * unit - (int(start[c0]) * unit & ~15)
                    assert furthest <= RS.REGION_BYTES, (S, D, es, unit, c0, furthest)
                    met.add(K)
    assert {4, 8, 12} <= met, met


@pytest.mark.parametrize("bits, interleaved, msb", [(8, True, False), (10, True, True), (16, True, True), (10, True, False), (10, False, True)])
def test_the_restatement_keeps_what_the_rule_promises(bits, interleaved, msb):
    rng = np.random.default_rng(bits)
    s = TS.shift_of(bits, msb)
    samples = R.make_clip(2, 16, 8, bits, rng)
    one, two = TS.pack(samples, bits, interleaved, msb, np.random.default_rng(1)), TS.pack(samples, bits, interleaved, msb, np.random.default_rng(2))
    a, b = RS.resize_surfaces(one, 8, 4, bits, interleaved, msb), RS.resize_surfaces(two, 8, 4, bits, interleaved, msb)
    planar = R.resize_clip(samples, 8, 4, bits)
    for x, y in zip(a, b):
        assert np.array_equal(x, y) and not np.any(x & ((1 << s) - 1))               # low bits neither matter nor survive
    for x, y in zip(TS.unpack(a, bits, interleaved, msb), planar):
        assert np.array_equal(x, y)                                                  # dst >> s, de-interleaved, is the planar resize
    same = RS.resize_surfaces(one, 16, 8, bits, interleaved, msb)
    for x, y in zip(same, one):
        assert np.array_equal(x >> s, y >> s) and not np.any(x & ((1 << s) - 1))     # equal sizes: the samples, low bits zero
