"""CPU side of the deband on decoder surfaces (amtgpu_deband_run_surfaces; DESIGN.md section 6f, "surfaces in kind"): what the composed
restatement (tests/deband_surfaces_ref.py) promises -- the source's low bits change nothing, the output's are zero, U and V do not mix,
and it is the planar restatement on the unpacked samples --; the interleaved UV table of the C++ plan (csrc/deband_plan.cpp, through the
stand-alone program tests/cpp/deband_interleave_test.cpp built with g++) against numpy; the entry point in the header, the binding and
the library; and the text the planar and the surface kernels share."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import deband_ref as R
import deband_surfaces_ref as DS
import temporal_nr_surfaces_ref as TS
from amtlib import ROOT

CSRC = os.path.join(ROOT, "amatsukaze_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")
# name: (bits, interleaved, msb)
KINDS = {"nv12": (8, True, False), "p010": (10, True, True), "p012": (12, True, True), "p016": (16, True, True), "il10": (10, True, False),
         "pmsb10": (10, False, True)}
W, H, N = 66, 38, 2


def samples_of(bits, seed=0):
    """a ramp in steps with noise of a few 8-bit units, on which threshold 2 keeps some pixels and filters others"""
    rng = np.random.default_rng(bits + seed)
    u = 1 << (bits - 8)
    dt = np.uint8 if bits <= 8 else np.uint16
    return tuple(((64 + (np.arange(pw)[None, None, :] // 8) * 2) * u + rng.integers(0, 4 * u + 1, (N, ph, pw))).astype(dt)
                 for pw, ph in ((W, H), (W // 2, H // 2), (W // 2, H // 2)))


@pytest.mark.parametrize("name", list(KINDS))
def test_the_restatement_is_the_planar_rule_on_samples_with_zero_low_bits_out(name):
    bits, il, msb = KINDS[name]
    s = TS.shift_of(bits, msb)
    samples = samples_of(bits)
    one, two = (TS.pack(samples, bits, il, msb, np.random.default_rng(k)) for k in (1, 2))
    assert len(one) == (2 if il else 3) and (not il or one[1].shape == (N, H // 2, W))
    if s:
        assert all(np.all(a & ((1 << s) - 1)) and np.mean(a != b) > 0.5 for a, b in zip(one, two))       # low bits everywhere, and other ones
    for sample, bf in ((0, True), (1, False), (2, True), (2, False)):
        a, b = (DS.deband_surfaces(p, bits, il, msb, 9, 2, sample, bf, seed=5) for p in (one, two))
        for x, y in zip(a, b):
            assert x.dtype == one[0].dtype and np.array_equal(x, y)                                      # the source's low bits change no byte
            assert not np.any(x & ((1 << s) - 1))                                                        # the output's are zero
        want = R.filter_clip(samples, bits, 9, 2, sample, bf, seed=5)
        for x, y in zip(TS.unpack(a, bits, il, msb), want):
            assert np.array_equal(x, y)
        assert any(0.02 < np.mean(x != y) < 0.98 for x, y in zip(want, samples))                         # some pixels kept, some filtered


@pytest.mark.parametrize("name", ["nv12", "p010", "pmsb10"])
def test_changing_one_component_changes_no_output_of_the_other(name):
    bits, il, msb = KINDS[name]
    Y, U, V = samples_of(bits)
    other = samples_of(bits, seed=77)
    base = TS.unpack(DS.deband_surfaces(TS.pack((Y, U, V), bits, il, msb), bits, il, msb, 25, 32767), bits, il, msb)
    newV = TS.unpack(DS.deband_surfaces(TS.pack((Y, U, other[2]), bits, il, msb), bits, il, msb, 25, 32767), bits, il, msb)
    newU = TS.unpack(DS.deband_surfaces(TS.pack((Y, other[1], V), bits, il, msb), bits, il, msb, 25, 32767), bits, il, msb)
    assert np.array_equal(newV[0], base[0]) and np.array_equal(newV[1], base[1]) and not np.array_equal(newV[2], base[2])
    assert np.array_equal(newU[0], base[0]) and np.array_equal(newU[2], base[2]) and not np.array_equal(newU[1], base[1])


@pytest.fixture(scope="module")
def interleave_test(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("deband_surfaces") / "deband_interleave_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(CPP, "deband_interleave_test.cpp"), os.path.join(CSRC, "deband_plan.cpp"),
                           "-o", out])
    return out


def test_the_interleave_program_checks_itself(interleave_test):
    r = subprocess.run([interleave_test], capture_output=True, text=True)
    assert r.returncode == 0 and "deband interleave ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("size, radius, seed", [((2, 2), 31, 0), ((8, 6), 25, 1), ((130, 98), 25, 0), ((290, 198), 31, 0xC0FFEE11)])
def test_the_interleaved_table_is_numpys(interleave_test, size, radius, seed):
    w, h = size
    Wc, Hc, Rc = w // 2, h // 2, R.plane_radius(1, radius)
    pitch = (w + 15) & ~15
    raw = subprocess.run([interleave_test, str(Wc), str(Hc), str(Rc), str(seed), str(pitch)], capture_output=True, check=True).stdout
    got = np.frombuffer(raw, np.int8).reshape(2, Hc, pitch)
    (dxU, dyU), (dxV, dyV) = R.table(1, Wc, Hc, Rc, seed), R.table(2, Wc, Hc, Rc, seed)
    assert np.array_equal(got[0, :, :w], np.stack([dxU, dxV], -1).reshape(Hc, w)) and np.array_equal(got[0, :, :w], DS.interleaved_table(dxU, dxV))
    assert np.array_equal(got[1, :, :w], np.stack([dyU, dyV], -1).reshape(Hc, w))
    assert not np.any(got[:, :, w:])                                                                     # rows padded to 16 with zeros


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_binding_and_library_carry_the_entry_point():
    from amatsukaze_amd import build as b
    b.build()
    raw = open(os.path.join(ROOT, "include", "amt_gpu.h")).read()
    proto = "int amtgpu_deband_run_surfaces(AmtGpuDeband* d, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes);"
    assert squeeze(proto) in squeeze(raw)
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", raw, re.M)                                       # an addition only
    from amatsukaze_amd import binding
    c_i, c_p = C.c_int, C.c_void_p
    assert binding.SIGNATURES["amtgpu_deband_run_surfaces"] == (c_i, [c_p, c_p, c_p, c_i]) == binding.SIGNATURES["amtgpu_deband_run"]
    assert {"deband_kernels.hip", "deband_surface_kernels.hip"} <= set(b.SOURCES)
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    assert {"amtgpu_deband_run", "amtgpu_deband_run_surfaces"} <= set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    lib = binding.load()
    assert lib.amtgpu_abi_version() == 5
    assert lib.amtgpu_deband_run_surfaces(None, None, None, 1) == 0                                      # no object: 0, and nothing is touched


def test_both_kernel_files_take_the_cell_from_one_header():
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f))}
    for fn in ("deband_cell", "deband_offsets", "deband_rows"):
        assert [f for f, t in files.items() if re.search(rf"__device__ __forceinline__ [^\n;]*\b{fn}\s*\(", t)] == ["deband_body.h"], fn
    for f in ("deband_kernels.hip", "deband_surface_kernels.hip"):
        assert re.search(r'^#include "deband_body\.h"', files[f], re.M), f
        assert re.search(r'^#include\s+[<"]([^>"]+)[>"]', files[f], re.M).group(1) == "build_knobs.h", f
    decl = [f for f, t in files.items() if re.search(r"hipError_t\s+launch_deband_surfaces\s*\([^)]*\)\s*;", t)]
    defs = [f for f, t in files.items() if re.search(r"hipError_t\s+launch_deband_surfaces\s*\([^)]*\)\s*\{", t)]
    assert decl == ["kernels.hpp"] and defs == ["deband_surface_kernels.hip"], (decl, defs)
    # both entry points run one set of checks, in the rule's order: side, side, in_kind, bytes, disjoint
    host = files["amt_gpu_deband.hip"]
    order = [host.index(t) for t in ('kPair.side("source"', 'kPair.side("destination"', "kDebandPair.in_kind(", "kPair.bytes(", "kPair.disjoint(")]
    assert order == sorted(order)
    # the UV plane's column halo fits the planar kernel's LDS pitch
    assert "static_assert(2 * (kDebandHalo >> 1) <= kDebandHalo" in files["kernels.hpp"]
