"""CPU side of the temporal noise reduction on decoder surfaces (amtgpu_temporal_nr_surfaces): the entry point in
the header, the binding and the library; the launcher declared once; the lane rule against a brute-force check; and the surfaces
checker (tests/temporal_nr_surfaces_ref.py) on the clips of tests/golden/temporal_nr_v1.npz packed into every kind their depth allows,
with random non-zero low bits -- unpacked, its results are what the compiled reference wrote, so the surfaces rule is pinned to the
reference through the packing and not only to a restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import temporal_nr_surfaces_ref as TS
from amtlib import ROOT

PROTOTYPE = ("int amtgpu_temporal_nr_surfaces(AmtGpuContext* ctx, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, "
             "int height, int out_first, int nout, int temporal_distance, int threshold, int interlaced, const AmtGpuSurfaces* dst);")
CSRC = os.path.join(ROOT, "amatsukaze_amd", "csrc")
NCASES = 6


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "temporal_nr_v1.npz"))


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_binding_and_library_carry_the_entry_point():
    from amatsukaze_amd import build as b
    b.build()
    raw = open(os.path.join(ROOT, "include", "amt_gpu.h")).read()
    text = squeeze(raw)
    assert squeeze(PROTOTYPE) in text
    # next to amtgpu_temporal_nr: no other prototype between the two
    between = text[text.index("int amtgpu_temporal_nr("):text.index("int amtgpu_temporal_nr_surfaces(")]
    assert between.count(";") == 1, between
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", raw, re.M)                        # an addition
    from amatsukaze_amd import binding
    c_i, c_p = C.c_int, C.c_void_p
    assert binding.SIGNATURES["amtgpu_temporal_nr_surfaces"] == binding.SIGNATURES["amtgpu_temporal_nr"] == (c_i, [c_p, c_p] + [c_i] * 10 + [c_p])
    assert {"temporal_nr_kernels.hip", "temporal_nr_surface_kernels.hip", "amt_gpu_tnr.hip"} <= set(b.SOURCES)
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    assert {"amtgpu_temporal_nr", "amtgpu_temporal_nr_surfaces"} <= set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    lib = binding.load()
    assert lib.amtgpu_abi_version() == 5
    assert lib.amtgpu_temporal_nr_surfaces.argtypes == binding.SIGNATURES["amtgpu_temporal_nr_surfaces"][1]


def test_the_launcher_is_declared_once_and_defined_once():
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f))}
    decl = [f for f, t in files.items() if re.search(r"hipError_t\s+launch_temporal_nr_surfaces\s*\([^)]*\)\s*;", t)]
    defs = [f for f, t in files.items() if re.search(r"hipError_t\s+launch_temporal_nr_surfaces\s*\([^)]*\)\s*\{", t)]
    assert decl == ["kernels.hpp"] and defs == ["temporal_nr_surface_kernels.hip"]
    sig = re.search(r"hipError_t\s+launch_temporal_nr_surfaces\s*\(([^)]*)\)\s*;", files["kernels.hpp"]).group(1)
    assert [a.split()[-1] for a in sig.split(",")] == ["st", "a", "interleaved", "shift", "nout"], sig
    assert [f for f, t in files.items() if re.search(r"\btemporal_nr_surface_vec16\(", t)] == ["amt_gpu_tnr.hip", "lane_rule.h"]
    # the planar file keeps its kernels to itself, and both entry points share one set of argument checks
    assert "temporal_nr_surfaces_kernel" not in files["temporal_nr_kernels.hip"]
    host = files["amt_gpu_tnr.hip"]
    assert len(re.findall(r"refuse\(\"temporal_distance must be", host)) == 1 and len(re.findall(r"\btemporal_nr\(c, src,", host)) == 2


def test_the_cell_and_the_reciprocal_table_are_defined_once():
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f))}
    # the cell: a function template whose name ends in _cell and whose first argument is the kernel's arguments
    cell = [(f, name) for f, t in files.items() for name in re.findall(r"\bvoid\s+(\w*_cell)\s*\(\s*const TemporalNRArgs&", t)]
    assert cell == [("temporal_nr_body.h", "tnr_cell")], cell
    table = [f for f, t in files.items() if re.search(r"__device__\s+const\s+\w+\s+k\w*Recip\w*\s*=", t)]
    loops = [f for f, t in files.items() if re.search(r"=\s*1\.f\s*/\s*\(float\)", t)]
    assert table == loops == ["temporal_nr_body.h"], (table, loops)
    both = ("temporal_nr_kernels.hip", "temporal_nr_surface_kernels.hip")
    assert [f for f, t in files.items() if re.search(r'^#include "temporal_nr_body\.h"', t, re.M)] == list(both)
    for f in both:
        assert re.search(r"\btnr_cell<", files[f]) and "__usad" not in files[f], f      # ... and use it, with no arithmetic of their own
    assert re.search(r"^#pragma once", files["temporal_nr_body.h"], re.M) and not re.search(r"^\s*__global__", files["temporal_nr_body.h"], re.M)


def test_the_lane_rule_against_brute_force(tmp_path):
    out = str(tmp_path / "temporal_nr_surface_lane_rule_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "temporal_nr_surface_lane_rule_test.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no difference" in r.stdout


def kinds_of_case(golden, k):
    """the kinds clip k goes through: every one of its depth in which its containers fit (a container above the depth's largest sample,
    which the planar call takes as stored, has no MSB-aligned form)"""
    bits = int(golden[f"c{k}_params"][0])
    top = max(int(golden[f"c{k}_{p}"].max()) for p in "YUV")
    return [kind for kind in TS.kinds_of(bits) if not TS.KINDS[kind][1] or top < (1 << bits)]


def test_the_golden_clips_reach_every_kind(golden):
    seen = {(int(golden[f"c{k}_params"][0]), kind) for k in range(NCASES) for kind in kinds_of_case(golden, k)}
    assert {(8, "nv12"), (10, "interleaved-lsb"), (14, "p0xx"), (14, "planar-msb"), (14, "interleaved-lsb"), (16, "p0xx"), (16, "interleaved-lsb")} <= seen, seen


@pytest.mark.parametrize("k", range(NCASES))
def test_the_packed_golden_clips_give_the_compiled_reference(golden, k):
    bits, d, thr, il = (int(v) for v in golden[f"c{k}_params"])
    samples = tuple(golden[f"c{k}_{p}"] for p in "YUV")
    want = tuple(golden[f"c{k}_{name}"] for name in ("oY", "oU", "oV"))
    kinds = kinds_of_case(golden, k)
    assert len(kinds) >= 2, kinds
    for kind in kinds:
        interleaved, msb = TS.KINDS[kind]
        s = TS.shift_of(bits, msb)
        low = (1 << s) - 1
        outs = []
        for seed in (k, k + 100):
            planes = TS.pack(samples, bits, interleaved, msb, np.random.default_rng(seed))
            assert len(planes) == (2 if interleaved else 3)
            if s:
                assert all(np.all(p & low) for p in planes), (kind, "a container without low bits")
            assert all(np.array_equal(a, b) for a, b in zip(TS.unpack(planes, bits, interleaved, msb), samples))
            got, count = TS.filter_surfaces(planes, d, thr, bits, interleaved, msb, bool(il))
            assert all(p.dtype == samples[0].dtype and not np.any(p & low) for p in got), (kind, "low bits in the output")
            for name, g, w in zip("YUV", TS.unpack(got, bits, interleaved, msb), want):
                assert g.dtype == w.dtype and np.array_equal(g, w), (k, kind, name, int(np.sum(g != w)))
            outs.append(got)
        assert all(np.array_equal(a, b) for a, b in zip(*outs)), (kind, "the output depends on the source's low bits")
