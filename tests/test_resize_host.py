"""CPU side of the resize (amtgpu_resize_*; DESIGN.md section 6e, "parity unpinned"): the C++ plan (csrc/resize_plan.cpp, through the
stand-alone program tests/cpp/resize_plan_test.cpp built with g++) against the numpy restatement (tests/resize_ref.py) entry for entry;
what the rule promises of every program; the known answers of the issue's table; the int32 check; the restatement's pixels against the
float64 evaluation of the continuous definition, within a bound derived here from the tables; the entry points in the header, the binding
and the library; and the lane rule against a brute-force check."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import resize_ref as R
from amtlib import ROOT

CSRC = os.path.join(ROOT, "amatsukaze_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")

# every (S, D) of an axis of a plane that tests/test_gpu_resize.py, tests/test_gpu_resize_far.py and tools/resize_bench.py resize ...
FRAMES = [((48, 36), (32, 24)), ((272, 48), (182, 34)), ((32, 24), (50, 40)), ((64, 32), (64, 32)), ((16, 8), (8, 4)), ((160, 24), (32, 16)),
          ((352, 240), (234, 160)), ((1920, 1080), (1280, 720))]
PAIRS = sorted({(s >> p, d >> p) for src, dst in FRAMES for s, d in zip(src, dst) for p in (0, 1)} | {(1440, 1280)})
KERNELS = ("blackman", "lanczos", "bilinear")


@pytest.fixture(scope="module")
def plan_test(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("resize") / "resize_plan_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(CPP, "resize_plan_test.cpp"), os.path.join(CSRC, "resize_plan.cpp"),
                           "-o", out])
    return out


@pytest.fixture(scope="module")
def cpp_programs(plan_test):
    """{(S, D, kernel): (K, start, C)} as the C++ plan makes them, default taps"""
    args = [str(v) for S, D in PAIRS for k in KERNELS for v in (S, D, R.KERNELS[k], 0)]
    out = subprocess.run([plan_test] + args, capture_output=True, text=True, check=True).stdout
    progs = {}
    for line in out.splitlines():
        head, start, coeff = line.split("|")
        S, D, kernel, _, K = (int(v) for v in head.split())
        progs[(S, D, KERNELS[kernel])] = (K, np.array(start.split(), np.int64), np.array(coeff.split(), np.int64).reshape(D, K))
    assert len(progs) == len(PAIRS) * len(KERNELS)
    return progs


def test_the_plan_program_checks_itself(plan_test):
    r = subprocess.run([plan_test], capture_output=True, text=True)
    assert r.returncode == 0 and "resize plan ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("kernel", KERNELS)
def test_cpp_and_numpy_tables_are_equal_entry_for_entry(cpp_programs, kernel):
    for S, D in PAIRS:
        K, start, Cf = cpp_programs[(S, D, kernel)]
        rK, rstart, rC = R.program(S, D, kernel)
        assert K == rK, (S, D, K, rK)
        assert np.array_equal(start, rstart), (S, D, "start")
        assert np.array_equal(Cf, rC), (S, D, "coefficients differ at", np.argwhere(Cf != rC)[:3].tolist())


# ... and the luma (S, D) of every frame tests/test_gpu_resize_spans.py resizes, widths and heights, with the two widths it must see refused
SPAN_FRAMES = [((1000, 8), (32, 8)), ((2000, 8), (66, 8)), ((1760, 8), (66, 8)), ((2048, 4), (32, 4)), ((2000, 8), (2, 8)), ((2002, 8), (2, 8)),
               ((1000, 8), (2, 8)), ((1002, 8), (2, 8)), ((2176, 12), (2080, 8)), ((1088, 12), (1040, 8)), ((1094, 12), (1046, 8)), ((100, 100), (38, 38)),
               ((48, 36), (32, 24)), ((272, 48), (182, 34))]
SPAN_PAIRS = sorted({(s >> p, d >> p) for src, dst in SPAN_FRAMES for s, d in zip(src, dst) for p in (0, 1)})


def test_the_columns_per_wave_port_is_the_cpp_rule(plan_test):
    """R.columns_per_wave, written from the rule's text, against resize_columns_per_wave as the library compiles it: every axis of the
    span tests and of the older ones, and S = 4 D .. 40 D in steps of 2 for D = 16, 34, 66 (ratios from where a run of 64 columns
    still fits to where not one column does), at containers of 1 and 2 bytes; and the explicit taps the span tests pass"""
    cases = [(S, D, "blackman", 0) for S, D in sorted(set(SPAN_PAIRS) | set(PAIRS))]
    cases += [(S, D, "blackman", 0) for D in (16, 34, 66) for S in range(4 * D, 40 * D + 1, 2)]
    cases += [(r * 66, 66, "blackman", 0) for r in (150, 200, 240, 250)]         # at 1 byte: runs of 4, 2 and 1 columns, and none
    cases += [(S, D, k, 0) for S, D in ((2000, 66), (1760, 66), (2048, 32), (272, 182)) for k in ("lanczos", "bilinear")]
    cases += [(S, D, "blackman", 8) for S, D in ((48, 32), (36, 24), (24, 16), (18, 12), (1000, 66))]
    cases = [c + (es,) for c in cases for es in (1, 2)]
    args = [str(v) for S, D, k, taps, es in cases for v in (S, D, R.KERNELS[k], taps, es)]
    out = subprocess.run([plan_test, "cpw"] + args, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases) >= 2 * 2091
    seen = set()
    for line, (S, D, k, taps, es) in zip(out, cases):
        cS, cD, ck, ctaps, ces, cK, ccpw = (int(v) for v in line.split())
        assert (cS, cD, ck, ctaps, ces) == (S, D, R.KERNELS[k], taps, es)
        cpw, K, spans = R.columns_per_wave(S, D, es, k, taps)
        assert (cpw, K) == (ccpw, cK), (S, D, k, taps, es, "port", cpw, K, "C++", ccpw, cK)
        assert (len(spans) == -(-D // cpw) and max(spans) + 48 <= 2048) if cpw else spans == ()
        seen.add(cpw)
    assert seen == {0, 1, 2, 4, 8, 16, 32, 64}                       # the sweep meets every answer the rule has


def test_the_ports_windows_are_the_programs():
    for S, D in SPAN_PAIRS + [(48, 32), (272, 182), (32, 50), (1920, 1280)]:
        for kernel, taps in (("blackman", None), ("lanczos", None), ("bilinear", None), ("blackman", 8)):
            if S * D > 300000 and kernel != "blackman":
                continue                                             # (the programs of the widest pairs once)
            K, start = R.windows(S, D, kernel, taps)
            pK, pstart, _ = R.program(S, D, kernel, taps)
            assert K == pK and np.array_equal(start, pstart), (S, D, kernel, taps)


def test_explicit_taps_reach_the_cpp_plan(plan_test):
    out = subprocess.run([plan_test, "48", "32", "1", "4", "48", "32", "0", "2"], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, (kernel, taps) in zip(out, (("lanczos", 4), ("blackman", 2))):
        head, start, coeff = line.split("|")
        K = int(head.split()[4])
        rK, rstart, rC = R.program(48, 32, kernel, taps)
        assert K == rK == 3 * taps and np.array_equal(np.array(start.split(), np.int64), rstart)
        assert np.array_equal(np.array(coeff.split(), np.int64).reshape(32, K), rC)


@pytest.mark.parametrize("kernel", KERNELS)
def test_rows_sum_to_one_and_windows_lie_inside(cpp_programs, kernel):
    for S, D in PAIRS:
        K, start, Cf = cpp_programs[(S, D, kernel)]
        assert np.all(Cf.sum(axis=1) == 16384), (S, D)
        assert start.min() >= 0 and start.max() + K <= S and np.all(np.diff(start) >= 0), (S, D)
        if S == D:
            assert np.all((Cf == 16384).sum(axis=1) == 1) and np.all((Cf != 0).sum(axis=1) == 1), (S, D)      # a single 16384 per row ...
            assert np.array_equal(start + np.argmax(Cf, axis=1), np.arange(S))                                 # ... at the sample itself


def test_the_known_answers_of_the_rule():
    pos = lambda Cf: int(np.where(Cf > 0, Cf, 0).sum(axis=1).max())
    neg = lambda Cf: int(np.where(Cf < 0, Cf, 0).sum(axis=1).min())
    for S, D in ((1920, 1280), (1080, 720)):
        K, start, Cf = R.program(S, D)
        assert (K, pos(Cf), neg(Cf)) == (12, 19144, -2760), (S, D, K, pos(Cf), neg(Cf))
    K, start, Cf = R.program(1920, 1280)
    assert int(start[63] + K - start[0]) == 101                        # a wave's 64 output columns read 101 source samples
    K, _, Cf = R.program(272, 182)
    assert (K, pos(Cf)) == (12, 19331)
    K, _, Cf = R.program(32, 50)
    assert (K, int(Cf.max())) == (8, 17723)
    assert R.program(1440, 1280)[0] == 9
    assert R.program(16, 8)[0] == 16
    K, start, Cf = R.program(8, 4)                                     # K0 = 16 folded into K = S = 8
    assert K == 8 and np.all(start == 0) and np.all(Cf.sum(axis=1) == 16384)
    K, _, Cf = R.program(64, 64)
    assert (K, pos(Cf), neg(Cf)) == (8, 16384, 0)
    assert R.program(48, 32, "lanczos")[0] == 9 and R.program(48, 32, "bilinear")[0] == 3
    # a constant stays constant, and equal sizes copy
    rng = np.random.default_rng(1)
    a = rng.integers(0, 1024, (1, 32, 64)).astype(np.uint16)
    assert np.array_equal(R.resize_plane(a, 64, 32, 10), a)
    for v in (0, 1, 1023):
        assert np.all(R.resize_plane(np.full((1, 36, 48), v, np.uint16), 32, 24, 10) == v)


def test_the_int32_check_passes_at_16_bits(cpp_programs):
    # what resize_program_fits_int32 computes, restated: it holds for every program here at 16 bits (the C++ program has checked its own
    # result for a subset, and that forged programs are refused: test_the_plan_program_checks_itself)
    for (S, D, kernel), (K, start, Cf) in cpp_programs.items():
        pos, neg = np.where(Cf > 0, Cf, 0).sum(axis=1).max(), np.where(Cf < 0, Cf, 0).sum(axis=1).min()
        assert int(pos) * 65535 + 8192 <= 2 ** 31 - 1 and int(neg) * 65535 + 8192 >= -2 ** 31, (S, D, kernel)


def stage_bound(S, D, kernel, maxv):
    """per output sample of one stage: (|integer result - float result| given equal inputs, the sum of |float weights|) -- the rounding's
    half unit plus the summed absolute coefficient error times the largest sample; and what an input error is multiplied by"""
    K, start, Cf = R.program(S, D, kernel)
    _, _, Wf = R.float_program(S, D, kernel)
    coeff_err = np.abs(Cf / 16384.0 - Wf).sum(axis=1)
    return 0.5 + coeff_err * maxv, np.abs(Wf).sum(axis=1)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("bits", [8, 10, 16])
def test_the_pixels_lie_within_the_derived_bound_of_the_continuous_definition(kernel, bits):
    """With x the exact stage input, x' the integer pipeline's (|x' - x| <= e), w the float weights and c / 16384 the quantised ones:
    |sum c/16384 x' - sum w x| <= sum |c/16384 - w| |x'| + sum |w| |x' - x| <= coeff_err * maxv + sum|w| * e, the rounding adds at most
    0.5, and the clamp to 0 .. maxv, applied to both, moves them no further apart.  e is 0 in front of the first stage and the first
    stage's bound (its largest over the row's columns) in front of the second."""
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    dt = np.uint8 if bits <= 8 else np.uint16
    for (sw, sh), (dw, dh) in FRAMES[:6]:
        noise = rng.integers(0, maxv + 1, (1, sh, sw)).astype(dt)
        edge_v = np.zeros((1, sh, sw), dt); edge_v[:, :, sw // 2:] = maxv
        edge_h = np.zeros((1, sh, sw), dt); edge_h[:, sh // 2:, :] = maxv
        b1, _ = stage_bound(sw, dw, kernel, maxv)                      # per output column
        b2, gain2 = stage_bound(sh, dh, kernel, maxv)                  # per output row
        bound = b2[:, None] + gain2[:, None] * b1[None, :]             # (dh, dw)
        assert bound.shape == (dh, dw) and bound.min() >= 0.5
        for what, plane in (("noise", noise), ("vertical edge", edge_v), ("horizontal edge", edge_h)):
            got = R.resize_plane(plane, dw, dh, bits, kernel).astype(np.float64)
            want = R.resize_plane_float(plane, dw, dh, bits, kernel)
            err = np.abs(got - want)[0]
            print(kernel, bits, (sw, sh), (dw, dh), what, "largest error %.3f, bound there %.3f, largest bound %.3f" %
                  (err.max(), bound.reshape(-1)[np.argmax(err)], bound.max()))
            assert np.all(err <= bound + 1e-9), (what, (sw, sh), (dw, dh), float((err - bound).max()))


PROTOTYPES = (
    "AmtGpuResize* amtgpu_resize_create(AmtGpuContext* ctx, int src_w, int src_h, int dst_w, int dst_h, int bits, int kernel, int taps, int64_t max_scratch_bytes);",
    "void amtgpu_resize_destroy(AmtGpuResize* r);",
    "int amtgpu_resize_run(AmtGpuResize* r, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes);",
    "int amtgpu_resize_get_program(AmtGpuResize* r, int plane, int axis, int* K, int* start, int* coeff);",
)


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_binding_and_library_carry_the_entry_points():
    from amatsukaze_amd import build as b
    b.build()
    import amatsukaze_amd as pkg
    raw = open(os.path.join(ROOT, "include", "amt_gpu.h")).read()
    for p in PROTOTYPES:
        assert squeeze(p) in squeeze(raw), p
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", raw, re.M)                        # additions only
    for name, v in (("BLACKMAN", 0), ("LANCZOS", 1), ("BILINEAR", 2)):
        assert re.search(rf"^#define AMTGPU_RESIZE_{name}\s+{v}\b", raw, re.M) and R.KERNELS[name.lower()] == v
    assert re.search(r"^#define AMTGPU_RESIZE_DEFAULT_SCRATCH_BYTES \(64ll << 20\)", raw, re.M)
    from amatsukaze_amd import api, binding
    c_i, c_p, c_i64 = C.c_int, C.c_void_p, C.c_int64
    assert binding.SIGNATURES["amtgpu_resize_create"] == (c_p, [c_p] + [c_i] * 7 + [c_i64])
    assert binding.SIGNATURES["amtgpu_resize_run"] == (c_i, [c_p, c_p, c_p, c_i])
    assert binding.SIGNATURES["amtgpu_resize_get_program"] == (c_i, [c_p, c_i, c_i, c_p, c_p, c_p])
    assert binding.SIGNATURES["amtgpu_resize_destroy"] == (None, [c_p])
    assert "Resizer" in pkg.__all__ and api.RESIZE_KERNELS == R.KERNELS
    assert all(callable(getattr(pkg.Resizer, m)) for m in ("run", "program", "close"))
    assert {"resize_kernels.hip", "amt_gpu_resize.hip", "resize_plan.cpp"} <= set(b.SOURCES)
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    assert {"amtgpu_resize_create", "amtgpu_resize_destroy", "amtgpu_resize_run", "amtgpu_resize_get_program"} <= set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    assert binding.load().amtgpu_abi_version() == 5


def test_the_launchers_are_declared_once_and_defined_once():
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f))}
    for name in ("launch_resize_h", "launch_resize_v"):
        decl = [f for f, t in files.items() if re.search(rf"hipError_t\s+{name}\s*\([^)]*\)\s*;", t)]
        defs = [f for f, t in files.items() if re.search(rf"hipError_t\s+{name}\s*\([^)]*\)\s*\{{", t)]
        assert decl == ["kernels.hpp"] and defs == ["resize_kernels.hip"], (name, decl, defs)
    assert [f for f, t in files.items() if re.search(r"\bresize_vec16\(", t)] == ["amt_gpu_resize.hip", "lane_rule.h"]
    # the plan pair holds no HIP
    for f in ("resize_plan.hpp", "resize_plan.cpp"):
        assert not re.search(r"hip/|__global__|__device__|hipError_t", files[f]), f


def test_the_lane_rule_against_brute_force(tmp_path):
    out = str(tmp_path / "resize_lane_rule_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(CPP, "resize_lane_rule_test.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no difference" in r.stdout
