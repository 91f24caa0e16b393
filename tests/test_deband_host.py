"""CPU side of the deband (amtgpu_deband_*; DESIGN.md section 6f, "parity unpinned"): the C++ offset tables (csrc/deband_plan.cpp, through
the stand-alone program tests/cpp/deband_plan_test.cpp built with g++) against the numpy restatement (tests/deband_ref.py) entry for
entry; what the rule promises of every table; the restatement's filter on constant planes, planes without room, threshold 0 and planted
pixels that tell the two blur_first settings apart, sit on the threshold, and sum to every remainder; the entry points in the header,
the binding and the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import deband_ref as R
from amtlib import ROOT

CSRC = os.path.join(ROOT, "amatsukaze_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")

SIZES = [(2, 2), (8, 6), (130, 34), (1280, 720)]
RADII = [1, 25, 31]
SEEDS = [0, 0xC0FFEE11]


@pytest.fixture(scope="module")
def plan_test(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("deband") / "deband_plan_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(CPP, "deband_plan_test.cpp"), os.path.join(CSRC, "deband_plan.cpp"),
                           "-o", out])
    return out


def test_the_plan_program_checks_itself(plan_test):
    r = subprocess.run([plan_test], capture_output=True, text=True)
    assert r.returncode == 0 and "deband plan ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_cpp_and_numpy_tables_are_equal_entry_for_entry(plan_test, size):
    w, h = size
    cases = [(p, *R.plane_size(p, w, h), R.plane_radius(p, radius), seed) for radius in RADII for seed in SEEDS for p in range(3)]
    raw = subprocess.run([plan_test] + [str(v) for c in cases for v in c], capture_output=True, check=True).stdout
    assert len(raw) == sum(2 * W * H for _, W, H, _, _ in cases)
    at = 0
    for p, W, H, Rp, seed in cases:
        got = np.frombuffer(raw, np.int8, 2 * W * H, at).reshape(2, H, W)
        at += 2 * W * H
        dx, dy = R.table(p, W, H, Rp, seed)
        for name, g, e in (("dx", got[0], dx), ("dy", got[1], dy)):
            assert np.array_equal(g, e), (size, "plane", p, "radius", Rp, "seed", seed, name, "differs at", np.argwhere(g != e)[:3].tolist())


@pytest.mark.parametrize("radius", RADII)
def test_offsets_stay_inside_lim_and_take_every_value(radius):
    for w, h in SIZES:
        for seed in SEEDS:
            seen = []
            for p in range(3):
                W, H = R.plane_size(p, w, h)
                Rp = R.plane_radius(p, radius)
                lim = R.lim_map(W, H, Rp)
                dx, dy = R.table(p, W, H, Rp, seed)
                assert dx.dtype == np.int8 and dx.shape == (H, W) == dy.shape
                assert np.all(np.abs(dx.astype(int)) <= lim) and np.all(np.abs(dy.astype(int)) <= lim), (w, h, p)
                if (w, h) == (1280, 720):
                    inner = lim == Rp
                    assert set(np.unique(dx[inner])) == set(range(-Rp, Rp + 1)) == set(np.unique(dy[inner])), (p, radius)
                seen.append((dx, dy))
            if (w, h) == (1280, 720) and radius > 1:
                # the planes' tables and the seeds' are tables of their own
                assert not np.array_equal(seen[1][0], seen[2][0])
                assert not np.array_equal(seen[0][0], R.table(0, w, h, radius, seed + 1)[0])


def test_the_known_answers_of_the_rule():
    assert int(R.mix(0)) == 0
    # mix, step by step, for one value
    v = 0x12345678
    v ^= v >> 16; v = (v * 0x7FEB352D) & R.M32; v ^= v >> 15; v = (v * 0x846CA68B) & R.M32; v ^= v >> 16
    assert int(R.mix(0x12345678)) == v
    # one entry, written out: plane 1, seed 5, (x, y) = (40, 30) of 64 x 48 at radius 12
    key = int(R.mix((5 + 0x9E3779B9 * 2) & R.M32))
    h = int(R.mix(key ^ (30 << 16 | 40)))
    lim = min(12, 40, 63 - 40, 30, 47 - 30)
    dx, dy = R.table(1, 64, 48, 12, 5)
    assert lim == 12 and int(dx[30, 40]) == (((h & 255) * 25) >> 8) - 12 and int(dy[30, 40]) == ((((h >> 8) & 255) * 25) >> 8) - 12
    assert R.plane_radius(0, 25) == 25 and R.plane_radius(1, 25) == 12 and R.plane_radius(2, 1) == 0


@pytest.mark.parametrize("bits", [8, 14, 16])
def test_constant_planes_stay_and_planes_without_room_copy(bits):
    dt = np.uint8 if bits <= 8 else np.uint16
    rng = np.random.default_rng(bits)
    for sample in (0, 1, 2):
        for bf in (True, False):
            for v in (0, 1, (1 << bits) - 1):
                planes = tuple(np.full((2, h, w), v, dt) for w, h in ((130, 34), (65, 17), (65, 17)))
                for o in R.filter_clip(planes, bits, 25, 1, sample, bf):
                    assert np.all(o == v)
            # 2 x 2: lim = 0 everywhere, in every plane; radius 1: the chroma planes' radius is 0
            tiny = tuple(rng.integers(0, 1 << bits, (3, h, w)).astype(dt) for w, h in ((2, 2), (1, 1), (1, 1)))
            for o, s in zip(R.filter_clip(tiny, bits, 31, 32767, sample, bf), tiny):
                assert np.array_equal(o, s)
            clip = tuple(rng.integers(0, 1 << bits, (2, h, w)).astype(dt) for w, h in ((34, 20), (17, 10), (17, 10)))
            out = R.filter_clip(clip, bits, 1, 32767, sample, bf)
            assert np.array_equal(out[1], clip[1]) and np.array_equal(out[2], clip[2]) and not np.array_equal(out[0], clip[0])
            assert np.array_equal(out[0][:, 0, :], clip[0][:, 0, :]) and np.array_equal(out[0][:, :, -1], clip[0][:, :, -1])      # lim = 0 on the rim


@pytest.mark.parametrize("sample", [0, 1, 2])
@pytest.mark.parametrize("bf", [True, False])
def test_threshold_0_changes_only_pixels_whose_average_is_the_pixel(sample, bf):
    rng = np.random.default_rng(3)
    s = rng.integers(0, 4, (3, 40, 60)).astype(np.uint8)              # few levels: many averages equal the centre
    dx, dy = R.table(0, 60, 40, 25, 1)
    out = R.filter_plane(s, dx, dy, 0, sample, bf)
    assert np.array_equal(out, s)
    c, p = R.references(s, dx, dy)
    avg = p[0] if sample == 0 else (p[0] + p[1] + 1) >> 1 if sample == 1 else (sum(p) + 2) >> 2
    assert 0.1 < np.mean(avg == c) < 0.9                               # both kinds of pixel are there


def planted(c, p, dt, at=(4, 4), d=(1, 2)):
    """a 9 x 9 plane of `c` whose pixel `at` has the offset d = (dx, dy) and the references p[0..4) there; every other offset is 0"""
    y, x = at
    dx, dy = np.zeros((9, 9), np.int8), np.zeros((9, 9), np.int8)
    dx[y, x], dy[y, x] = d
    s = np.full((9, 9), c, dt)
    for v, (yy, xx) in zip(p, ((y + d[1], x + d[0]), (y - d[1], x - d[0]), (y + d[0], x - d[1]), (y - d[0], x + d[1]))):
        s[yy, xx] = v
    return s, dx, dy


def out_at(s, dx, dy, thresh, sample, bf, at=(4, 4)):
    o = R.filter_plane(s, dx, dy, thresh, sample, bf)
    rest = np.ones(s.shape, bool)
    rest[at] = False
    assert np.array_equal(o[rest], s[rest])                            # offset 0 elsewhere: every reference is the pixel itself
    return int(o[at])


def test_the_four_references_are_where_the_rule_puts_them():
    # each reference alone carries the sum: 4 * 25 + 2 >> 2 = 25 above the centre's 0 only from its own place
    for k in range(4):
        p = [0, 0, 0, 0]
        p[k] = 100
        s, dx, dy = planted(0, p, np.uint8)
        assert np.argwhere(s == 100).tolist() == [list(((6, 5), (2, 3), (5, 2), (3, 6))[k])]      # (y, x) of p0 .. p3 for (dx, dy) = (1, 2) at (4, 4)
        assert out_at(s, dx, dy, 255, 2, True) == 25
        assert out_at(s, dx, dy, 255, 1, True) == (50 if k < 2 else 0)
        assert out_at(s, dx, dy, 255, 0, True) == (100 if k == 0 else 0)


@pytest.mark.parametrize("bits", [8, 14, 16])
def test_a_planted_pixel_tells_blur_first_from_not(bits):
    dt = np.uint8 if bits <= 8 else np.uint16
    t = 1 << (bits - 8)                                                # threshold 1
    c = 100 * t
    # the average lies within thresh, one reference outside: 4 t above the centre moves the average by exactly t
    s, dx, dy = planted(c, [c, c, c, c + 4 * t], dt)
    assert out_at(s, dx, dy, t, 2, True) == c + t
    assert out_at(s, dx, dy, t, 2, False) == c
    s, dx, dy = planted(c, [c, c + 2 * t, c, c], dt)
    assert out_at(s, dx, dy, t, 1, True) == c + t
    assert out_at(s, dx, dy, t, 1, False) == c
    # every reference within thresh: both settings filter
    s, dx, dy = planted(c, [c + t, c + t, c + t, c + t], dt)
    assert out_at(s, dx, dy, t, 2, True) == c + t == out_at(s, dx, dy, t, 2, False)


@pytest.mark.parametrize("bits, threshold", [(8, 1), (8, 3), (10, 1), (14, 1), (16, 2), (16, 127)])
def test_planted_pixels_on_the_threshold_and_one_beyond(bits, threshold):
    dt = np.uint8 if bits <= 8 else np.uint16
    t = threshold << (bits - 8)
    c = (1 << bits) // 2
    for sign in (1, -1):
        for sample in (0, 1, 2):
            for bf in (True, False):
                on, off = c + sign * t, c + sign * (t + 1)
                s, dx, dy = planted(c, [on] * 4, dt)
                assert out_at(s, dx, dy, t, sample, bf) == on, (sign, sample, bf)            # |avg - c| = thresh: filtered
                s, dx, dy = planted(c, [off] * 4, dt)
                assert out_at(s, dx, dy, t, sample, bf) == c, (sign, sample, bf)             # thresh + 1: kept


def test_the_rounding_for_every_remainder():
    for bits, c in ((8, 40), (16, 65531), (16, 0)):
        dt = np.uint8 if bits <= 8 else np.uint16
        for k in range(4):                                             # p0 + p1 + p2 + p3 = 4 c + k
            for place in range(4):
                p = [c] * 4
                p[place] += k
                s, dx, dy = planted(c, p, dt)
                assert out_at(s, dx, dy, 1 << 15, 2, True) == c + (1 if k >= 2 else 0), (bits, c, k)
        for k in range(2):                                             # p0 + p1 = 2 c + k
            for place in range(2):
                p = [c] * 4
                p[place] += k
                s, dx, dy = planted(c, p, dt)
                assert out_at(s, dx, dy, 1 << 15, 1, True) == c + k, (bits, c, k)
    # four containers of 65 535: the sum needs 18 bits
    s, dx, dy = planted(65535, [65535] * 4, np.uint16)
    assert out_at(s, dx, dy, 0, 2, True) == 65535
    s, dx, dy = planted(0, [65535] * 4, np.uint16)
    assert out_at(s, dx, dy, 65535, 2, True) == 65535 and out_at(s, dx, dy, 65534, 2, True) == 0


def test_a_ramp_in_steps_gains_levels():
    # 14 bits in 8-bit steps of 64: the filter's only purpose
    ramp = ((np.arange(512) // 64) * 64 + 4096).astype(np.uint16)
    s = np.broadcast_to(ramp, (128, 512)).copy()
    dx, dy = R.table(0, 512, 128, 25, 0)
    out = R.filter_plane(s, dx, dy, 1 << 6, 2, True)
    assert len(np.unique(s)) == 8 and len(np.unique(out)) > 16, len(np.unique(out))


PROTOTYPES = (
    "AmtGpuDeband* amtgpu_deband_create(AmtGpuContext* ctx, int width, int height, int bits, int radius, int threshold, int sample, int blur_first, uint32_t seed);",
    "void amtgpu_deband_destroy(AmtGpuDeband* d);",
    "int amtgpu_deband_run(AmtGpuDeband* d, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes);",
    "int amtgpu_deband_get_offsets(AmtGpuDeband* d, int plane, int8_t* dx, int8_t* dy);",
    "int amtgpu_deband_set_offsets(AmtGpuDeband* d, int plane, const int8_t* dx, const int8_t* dy);",
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
    from amatsukaze_amd import binding
    c_i, c_p = C.c_int, C.c_void_p
    assert binding.SIGNATURES["amtgpu_deband_create"] == (c_p, [c_p] + [c_i] * 7 + [C.c_uint32])
    assert binding.SIGNATURES["amtgpu_deband_run"] == (c_i, [c_p, c_p, c_p, c_i])
    assert binding.SIGNATURES["amtgpu_deband_get_offsets"] == (c_i, [c_p, c_i, c_p, c_p]) == binding.SIGNATURES["amtgpu_deband_set_offsets"]
    assert binding.SIGNATURES["amtgpu_deband_destroy"] == (None, [c_p])
    assert "Debander" in pkg.__all__
    assert all(callable(getattr(pkg.Debander, m)) for m in ("run", "offsets", "set_offsets", "close"))
    assert {"amt_gpu_deband.hip", "deband_kernels.hip", "deband_plan.cpp"} <= set(b.SOURCES)
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    assert {"amtgpu_deband_create", "amtgpu_deband_destroy", "amtgpu_deband_run", "amtgpu_deband_get_offsets", "amtgpu_deband_set_offsets"} <= \
        set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    assert binding.load().amtgpu_abi_version() == 5


def test_the_launcher_is_declared_once_and_defined_once():
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f))}
    decl = [f for f, t in files.items() if re.search(r"hipError_t\s+launch_deband\s*\([^)]*\)\s*;", t)]
    defs = [f for f, t in files.items() if re.search(r"hipError_t\s+launch_deband\s*\([^)]*\)\s*\{", t)]
    assert decl == ["kernels.hpp"] and defs == ["deband_kernels.hip"], (decl, defs)
    assert [f for f, t in files.items() if re.search(r"\bdeband_vec16\(", t)] == ["amt_gpu_deband.hip", "lane_rule.h"]
    for f in ("amt_gpu_deband.hip", "deband_kernels.hip", "deband_plan.cpp"):
        assert re.search(r'^#include\s+[<"]([^>"]+)[>"]', files[f], re.M).group(1) == "build_knobs.h", f
    # the plan pair holds no HIP
    for f in ("deband_plan.hpp", "deband_plan.cpp"):
        assert not re.search(r"hip/|__global__|__device__|hipError_t", files[f]), f
    # the tile constants the GPU and ISA tests mirror
    assert re.search(r"constexpr int kDebandTileW = 128, kDebandTileH = 96;", files["kernels.hpp"])
    assert re.search(r"constexpr int kDebandHalo = 31;", files["kernels.hpp"])


def test_the_lane_rule_takes_every_operand(tmp_path):
    """deband_vec16 against the definition: 16 divides every base, stride and pitch of all four plane kinds"""
    out = str(tmp_path / "deband_lane_rule_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(CPP, "deband_lane_rule_test.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no difference" in r.stdout
