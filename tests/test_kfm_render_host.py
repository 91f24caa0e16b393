"""CPU side of the cadence renderer: the render plan on hand-written cadence / phase arrays against the numpy restatement
(tests/kfm_render_ref.py) and against the durations file, the plan call's capacity contract, and the two entry points in the header, the
binding and the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kfm_render_ref as R
from amtlib import ROOT

PROTOTYPES = (
    "int amtgpu_kfm_render_plan(const uint8_t* cadence, const uint8_t* phase, int nframes, AmtGpuRenderFrame* out, int cap, int* nout);",
    "int amtgpu_kfm_render(AmtGpuContext* ctx, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height, "
    "const AmtGpuRenderFrame* plan, int nout, int thresh, const AmtGpuSurfaces* dst);",
)
NAMES = tuple(re.search(r"(amtgpu_\w+)\(", p).group(1) for p in PROTOTYPES)

I, F, P = R.CAD_60I, R.CAD_24P, R.CAD_30P
CYCLE = [(F, k) for k in range(5)]
# (cadence, phase) per frame
CLIPS = {
    "one-complete-cycle": CYCLE,
    "two-cycles-then-one-cut-by-the-clip-end": CYCLE * 2 + CYCLE[:4],
    "cycle-starting-at-phase-2": [(F, 2), (F, 3), (F, 4)] + CYCLE + [(F, 0), (F, 1)],
    "60i-and-30p-runs": [(I, 0)] * 3 + [(P, 0)] * 4 + [(I, 0)] + [(P, 0)],
    "broken-phase-inside-24p": CYCLE[:3] + [(F, 4), (F, 0)] + CYCLE + [(F, 0), (F, 1), (F, 1), (F, 3), (F, 4)],
    "a-60i-frame-inside-a-cycle": CYCLE[:2] + [(I, 2)] + CYCLE[3:] + CYCLE,
    "30p-with-stray-phases": [(P, 0), (P, 1), (P, 2), (P, 3), (P, 4)],
    "mixed": [(I, 0)] * 2 + CYCLE + [(P, 0)] * 2 + CYCLE + [(I, 0)] + CYCLE[:2],
    "single-frames": [(F, 0)],
}


@pytest.fixture(scope="module")
def A():
    from amatsukaze_amd import build as b
    b.build()
    import amatsukaze_amd
    return amatsukaze_amd


def arrays(clip):
    return np.array([c for c, _ in clip], np.uint8), np.array([p for _, p in clip], np.uint8)


@pytest.mark.parametrize("name", list(CLIPS))
def test_plan_is_the_numpy_plan_and_its_ticks_are_the_durations_file(A, tmp_path, name):
    cad, ph = arrays(CLIPS[name])
    plan = A.kfm_render_plan(cad, ph)
    want = R.render_plan_ref(cad, ph)
    assert plan.dtype.names == ("kind", "top", "bottom", "ticks") and plan.dtype.itemsize == 16
    assert [tuple(int(v) for v in e) for e in plan] == want
    # the durations file of the same arrays, entry for entry
    from amatsukaze_amd import binding
    lib = binding.load()
    path, k = str(tmp_path / "d.duration.txt"), C.c_int()
    assert lib.amtgpu_kfm_write_durations(cad.ctypes.data_as(C.c_void_p), ph.ctypes.data_as(C.c_void_p), len(cad), path.encode(), C.byref(k)) == 1
    durations = [int(l) for l in open(path).read().split()]
    assert k.value == len(durations) == len(plan) and durations == [int(t) for t in plan["ticks"]]
    assert int(plan["ticks"].sum()) == 2 * len(cad)


def test_the_named_shapes_are_in_the_plans(A):
    plan = lambda name: [tuple(int(v) for v in e) for e in A.kfm_render_plan(*arrays(CLIPS[name]))]
    W, T, B = R.WEAVE, R.BOB_TOP, R.BOB_BOTTOM
    assert plan("one-complete-cycle") == [(W, 0, 0, 2), (W, 1, 1, 3), (W, 3, 2, 2), (W, 4, 4, 3)]
    cut = plan("two-cycles-then-one-cut-by-the-clip-end")
    assert cut[4:8] == [(W, 5, 5, 2), (W, 6, 6, 3), (W, 8, 7, 2), (W, 9, 9, 3)] and cut[8:] == [(W, n, n, 2) for n in range(10, 14)]
    ph2 = plan("cycle-starting-at-phase-2")
    assert ph2[:3] == [(W, n, n, 2) for n in range(3)] and ph2[3:7] == [(W, 3, 3, 2), (W, 4, 4, 3), (W, 6, 5, 2), (W, 7, 7, 3)]
    assert ph2[7:] == [(W, 8, 8, 2), (W, 9, 9, 2)]
    runs = plan("60i-and-30p-runs")
    assert runs[:6] == [(T, 0, 0, 1), (B, 0, 0, 1), (T, 1, 1, 1), (B, 1, 1, 1), (T, 2, 2, 1), (B, 2, 2, 1)]
    assert runs[6:10] == [(W, n, n, 2) for n in range(3, 7)] and runs[10:] == [(T, 7, 7, 1), (B, 7, 7, 1), (W, 8, 8, 2)]
    broken = plan("broken-phase-inside-24p")
    # phases 0 1 2 4 0: no cycle at 0; the phase-0 frame 4 is followed by 0 1 2 3: none either; frames 5..9 are whole; 0 1 1 3 4 is not
    assert broken[:5] == [(W, n, n, 2) for n in range(5)]
    assert broken[5:9] == [(W, 5, 5, 2), (W, 6, 6, 3), (W, 8, 7, 2), (W, 9, 9, 3)]
    assert broken[9:] == [(W, n, n, 2) for n in range(10, 15)]
    inside = plan("a-60i-frame-inside-a-cycle")
    assert inside[:2] == [(W, 0, 0, 2), (W, 1, 1, 2)] and inside[2:4] == [(T, 2, 2, 1), (B, 2, 2, 1)]


def test_plan_capacity_contract(A):
    from amatsukaze_amd import binding
    lib = binding.load()
    cad, ph = arrays(CLIPS["mixed"])
    want = R.render_plan_ref(cad, ph)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    out, k = np.full(len(want) + 2, -7, R.RENDER_FRAME), C.c_int(-1)
    # cap too small: 0, the count needed, nothing written
    assert lib.amtgpu_kfm_render_plan(p(cad), p(ph), len(cad), p(out), len(want) - 1, C.byref(k)) == 0
    assert k.value == len(want) and (out["kind"] == -7).all() and (out["ticks"] == -7).all()
    assert lib.amtgpu_kfm_render_plan(p(cad), p(ph), len(cad), None, 0, C.byref(k)) == 0 and k.value == len(want)
    # exactly enough: 1, and nothing behind the last entry is touched
    assert lib.amtgpu_kfm_render_plan(p(cad), p(ph), len(cad), p(out), len(want), C.byref(k)) == 1 and k.value == len(want)
    assert [tuple(int(v) for v in e) for e in out[:len(want)]] == want and (out["kind"][len(want):] == -7).all()
    # no frames: 1 with *nout = 0, whatever the pointers
    k = C.c_int(-1)
    assert lib.amtgpu_kfm_render_plan(None, None, 0, None, 0, C.byref(k)) == 1 and k.value == 0
    assert len(A.kfm_render_plan([], [])) == 0
    assert lib.amtgpu_kfm_render_plan(p(cad), p(ph), -1, p(out), len(out), C.byref(k)) == 0
    with pytest.raises(A.AmtError):
        A.kfm_render_plan([0, 0], [0])


def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_binding_and_library_carry_the_entry_points(A):
    raw = open(os.path.join(ROOT, "include", "amt_gpu.h")).read()
    hdr = squeeze(raw)
    for proto in PROTOTYPES:
        assert squeeze(proto) in hdr, proto
    assert "typedef struct AmtGpuRenderFrame { int32_t kind, top, bottom, ticks; } AmtGpuRenderFrame;" in hdr
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", raw, re.M)            # additions only
    for name, value in (("WEAVE", 0), ("BOB_TOP", 1), ("BOB_BOTTOM", 2)):
        assert re.search(rf"^#define AMTGPU_RENDER_{name}\s+{value}\b", raw, re.M), name
    from amatsukaze_amd import api, binding, build as b
    c_i, c_p = C.c_int, C.c_void_p
    want = {
        "amtgpu_kfm_render_plan": (c_i, [c_p, c_p, c_i, c_p, c_i, c_p]),
        "amtgpu_kfm_render": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p, c_i, c_i, c_p]),
    }
    assert set(want) == set(NAMES)
    for name, sig in want.items():
        assert binding.SIGNATURES[name] == sig, name
    assert C.sizeof(binding.RenderFrame) == 16 == api.RENDER_FRAME.itemsize
    assert [f[0] for f in binding.RenderFrame._fields_] == list(api.RENDER_FRAME.names)
    assert {"render_kernels.hip", "amt_gpu_render.hip"} <= set(b.SOURCES)
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    assert set(NAMES) <= exported
    assert binding.load().amtgpu_abi_version() == 5
    for name in ("kfm_render_plan", "kfm_render"):
        assert name in A.__all__ and hasattr(A, name)
    # the launcher is declared once, in kernels.hpp
    csrc = os.path.join(ROOT, "amatsukaze_amd", "csrc")
    decl = [f for f in sorted(os.listdir(csrc)) if re.search(r"hipError_t\s+launch_kfm_render\s*\([^)]*\)\s*;", open(os.path.join(csrc, f)).read())]
    assert decl == ["kernels.hpp"]


def test_the_third_picture_of_a_cycle_is_the_generator_film_picture():
    """the plan's WEAVE(top n + 3, bottom n + 2) against the synthetic generator: 3:2 frames 5g .. 5g + 4 hold film pictures 4g .. 4g + 3,
    and the "30p" frame 2g + 1 is film picture 4g + 2 whole"""
    import amt_synth as S
    W, H, seed = 96, 36, 0x5EED0003
    clip = np.stack([S.frame_planes_np(n, W, H, seed, 8, "24p")[0] for n in range(5)])[None]
    planes = (clip[0], clip[0, :, ::2, ::2], clip[0, :, ::2, ::2])
    plan = R.render_plan_ref([F] * 5, range(5))
    Y = R.render_ref(planes, plan, -1)[0]
    assert np.array_equal(Y[2], S.frame_planes_np(1, W, H, seed, 8, "30p")[0])
    assert not np.array_equal(clip[0, 2], Y[2]) and not np.array_equal(clip[0, 3], Y[2])
    for k, n in ((0, 0), (1, 1), (3, 4)):
        assert np.array_equal(Y[k], clip[0, n])
