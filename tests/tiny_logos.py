"""Logos at and below the size limits by which the evaluation code picks its kernel form, the clips they sit in, and the CPU oracle's
answers for them.  Checker side only: importable without a GPU (tests/test_tiny_logos_host.py, tests/test_gpu_tiny_logos.py).

The limits (amatsukaze_amd/csrc/eval_engine.hip pair_eligible / tiles_usable, eval_tiles.hpp build_tile_plan): the tile kernels take an
engine when EVERY logo of it has w >= 6, w even, h >= 5 and at least one mask pixel; a mask pixel needs 2 <= x < w - 2 and 2 <= y < h - 2
(CorrelationScore walks the interior only), and AMTAnalyzeLogo evaluates three logos -- deinterlaced (w x h), top and bottom field
(w x h / 2).  That gives three regimes:

    none    no logo has a mask pixel: every record is 0 / blackScore = 0 / 0
    mixed   the deinterlaced logo has mask pixels, the field logos (3 or 4 rows) have none
    all     all three have; the field logos of the h = 10 cases have exactly one mask row

amt_synth.make_logo keeps an 8-pixel ring of every logo clear, so its alpha is 0 everywhere at these sizes; tiny_logo draws alpha
uniformly instead.  Every clip has nine frames of noise over the whole depth with the logo blended in at an opacity that changes from
frame to frame (0, 1 and values between; frames 3 and 7 differ between their fields).  The samples INSIDE the rectangle depend on the
logo size and the depth only, not on where the rectangle lies: DeintY / CopyY read nothing else, so one size has the same records at
every placement, and CLIP_SEEDS below is one number per (size, depth)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from amtlib import Oracle, _ptr

GROUPS = {
    "none": ((2, 2), (4, 4), (4, 10), (10, 4)),
    "mixed": ((6, 6), (6, 8)),
    "all": ((6, 10), (8, 10), (10, 10), (130, 10)),
}
CASES = [(g, w, h) for g in ("none", "mixed", "all") for (w, h) in GROUPS[g]]
RATIOS = (0.35, 1.0)
DEPTHS = (8, 10, 16)
N_FRAMES = 9
PLACEMENTS = ("inside", "top_left", "bottom_right")
GUARD = 64 * 1024                    # containers in front of, between and behind the planes of a guarded clip
# opacity of the logo in the (top, bottom) field of each frame
OPACITY = ((0.0, 0.0), (0.2, 0.2), (0.0, 0.0), (0.3, 0.8), (0.5, 0.5), (1.0, 1.0), (0.8, 0.8), (1.0, 0.4), (1.0, 1.0))
FIELD_FRAMES = (3, 7)
assert len(OPACITY) == N_FRAMES and all((a != b) == (i in FIELD_FRAMES) for i, (a, b) in enumerate(OPACITY))


def case_id(case):
    return "%s-%dx%d" % case


def group_of(w, h):
    return next(g for g, sizes in GROUPS.items() if (w, h) in sizes)


def logo_seed(w, h):
    return 0x7100000 + 1000 * w + h


def tiny_logo_planes(w, h, seed):
    """(data, alpha, alphaUV): alpha uniform in 0.05 .. 0.6 per luma pixel, chroma alpha its 2 x 2 mean, amt_synth.make_logo's colours
    and plane layout (aY, bY, aU, bU, aV, bV: AMTLogo.hpp:204-212)"""
    alpha = np.random.default_rng(seed).uniform(0.05, 0.6, (h, w))
    cY, cC = 235.0 / 255.0, 128.0 / 255.0
    aY = (1.0 / (1.0 - alpha)).astype(np.float32)
    bY = (-alpha * cY / (1.0 - alpha)).astype(np.float32)
    alphaUV = alpha.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    aC = (1.0 / (1.0 - alphaUV)).astype(np.float32)
    bC = (-alphaUV * cC / (1.0 - alphaUV)).astype(np.float32)
    data = np.concatenate([aY.ravel(), bY.ravel(), aC.ravel(), bC.ravel(), aC.ravel(), bC.ravel()]).astype(np.float32)
    return data, alpha, alphaUV


def tiny_logo(w, h, seed=None):
    return tiny_logo_planes(w, h, logo_seed(w, h) if seed is None else seed)[0]


def geometry(w, h, placement):
    """(W, H, X, Y0, pitch padding): "inside" -- (224, 18) of a 352 x 240 frame whose rows carry 32 containers of padding (16 in chroma):
    everything a kernel touches around the rectangle is inside the frame (the 130 wide logo would end at column 354 of 352 there and
    sits at (192, 18)); the corners -- flush in an unpadded frame (pitch == width) just large enough for it"""
    if placement == "inside":
        return 352, 240, (224 if w <= 96 else 192), 18, 32
    W, H = (160 if w > 32 else 32), 16
    assert w <= W and h <= H
    return (W, H, 0, 0, 0) if placement == "top_left" else (W, H, W - w, H - h, 0)


# One seed per (size, depth) of the "all" group, the first of 0, 1, 2 ... for which the ORACLE's CalcFade gives, at maskratio 0.35 and at
# 1.0, a field-mode fade pair and a pair off {0, 1} (tests/test_tiny_logos_host.py asserts both): with a dozen mask pixels under noise
# over the whole depth the argmins are close to random, so a clip has them by its draw, not by its design.  Chosen from the oracle's
# output alone, before any kernel ran.
CLIP_SEEDS = {(6, 10, 8): 9, (6, 10, 10): 10, (6, 10, 16): 2, (8, 10, 8): 1, (8, 10, 10): 1, (8, 10, 16): 3,
              (10, 10, 8): 2, (10, 10, 10): 1, (10, 10, 16): 0, (130, 10, 8): 1, (130, 10, 10): 0, (130, 10, 16): 3}


def clip_seed(w, h, bits):
    return 0x5EED7000 + 64 * CLIP_SEEDS.get((w, h, bits), 0) + {8: 0, 10: 1, 16: 2}[bits] + 4096 * (1000 * w + h)


def rect_samples(w, h, bits, seed=None):
    """the rectangle's samples of the nine frames, (Y (9, h, w), U, V (9, h / 2, w / 2)): noise over the whole depth with the logo blended
    in -- obs = (1 - o alpha) bg + o alpha c maxv, o the frame's opacity in the row's field"""
    maxv = (1 << bits) - 1
    _, alpha, alphaUV = tiny_logo_planes(w, h, logo_seed(w, h))
    rng = np.random.default_rng(clip_seed(w, h, bits) if seed is None else seed)
    dt = np.uint8 if bits <= 8 else np.uint16
    out = []
    for (pw, ph, al, col) in ((w, h, alpha, 235.0 / 255.0), (w // 2, h // 2, alphaUV, 128.0 / 255.0), (w // 2, h // 2, alphaUV, 128.0 / 255.0)):
        bg = rng.integers(0, maxv + 1, (N_FRAMES, ph, pw)).astype(np.float64)
        op = np.array([[OPACITY[n][y & 1] for y in range(ph)] for n in range(N_FRAMES)])[:, :, None]
        a = al[None] * op
        out.append(np.clip(np.rint((1 - a) * bg + a * col * maxv), 0, maxv).astype(dt))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tiny_clip(w, h, bits, placement):
    """{"Y", "U", "V"}: (9, H, pitch) / (9, H / 2, pitch / 2) frames of noise over the whole depth, row padding included, with
    rect_samples at the placement's rectangle.  Read-only (shared between tests)."""
    W, H, X, Y0, pad = geometry(w, h, placement)
    maxv = (1 << bits) - 1
    dt = np.uint8 if bits <= 8 else np.uint16
    rng = np.random.default_rng(clip_seed(w, h, bits) + 1 + PLACEMENTS.index(placement))
    clip = {"Y": rng.integers(0, maxv + 1, (N_FRAMES, H, W + pad)).astype(dt),
            "U": rng.integers(0, maxv + 1, (N_FRAMES, H // 2, W // 2 + pad // 2)).astype(dt),
            "V": rng.integers(0, maxv + 1, (N_FRAMES, H // 2, W // 2 + pad // 2)).astype(dt)}
    rY, rU, rV = rect_samples(w, h, bits)
    clip["Y"][:, Y0:Y0 + h, X:X + w] = rY
    clip["U"][:, Y0 // 2:(Y0 + h) // 2, X // 2:(X + w) // 2] = rU
    clip["V"][:, Y0 // 2:(Y0 + h) // 2, X // 2:(X + w) // 2] = rV
    for v in clip.values():
        v.setflags(write=False)
    return clip


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle():
    return Oracle()


def oracle_logo(w, h, placement, data=None):
    W, H, X, Y0, _ = geometry(w, h, placement)
    return oracle().make_logo(tiny_logo(w, h) if data is None else data, w, h, W, H, X, Y0)


def oracle_eval_logos(lo, ratio):
    """(deinterlaced, top field, bottom field) with their masks made, as AMTAnalyzeLogo's constructor does"""
    L = oracle().lib
    d = L.orc_logo_deint(lo); L.orc_logo_create_mask(d, ratio, 1)
    t = L.orc_logo_field(lo, 0); L.orc_logo_create_mask(t, ratio, 1)
    b = L.orc_logo_field(lo, 1); L.orc_logo_create_mask(b, ratio, 1)
    return d, t, b


def mask_counts(w, h, ratio):
    """mask pixels with a whole 5 x 5 window (the tables' `count`) of the deinterlaced, top field and bottom field logo"""
    return tuple(int(oracle().logo_info(x)[9]) for x in oracle_eval_logos(oracle_logo(w, h, "inside"), ratio))


def oracle_scan(handles, Y, bits, W, H):
    """orc_logoframe_scan over deinterlaced logos with their masks made: (frames, logos, 2)"""
    n, nl = Y.shape[0], len(handles)
    out = np.zeros(n * nl * 2, np.float32)
    oracle().lib.orc_logoframe_scan((C.c_void_p * nl)(*handles), nl, _ptr(Y), Y.strides[0], Y.shape[2], bits, W, H, n, _ptr(out))
    return out.reshape(n, nl, 2)


def oracle_fades(records):
    """CalcFade (no logoframe file) of every frame: (frames, 2)"""
    an = np.ascontiguousarray(records, np.float32)
    n = an.shape[0]
    out = np.zeros((n, 2), np.float32)
    for i in range(n):
        ft, fb = C.c_float(), C.c_float()
        oracle().lib.orc_calc_fade(None, 0, 16, _ptr(an), n, i, C.byref(ft), C.byref(fb))
        out[i] = (ft.value, fb.value)
    return out


def oracle_erase(lo, clip, bits, fades):
    """the oracle's Delogo, frame by frame, on a copy of the clip"""
    want = {k: np.array(clip[k], copy=True) for k in "YUV"}
    for i in range(want["Y"].shape[0]):
        oracle().lib.orc_erase_frame(lo, _ptr(want["Y"][i]), _ptr(want["U"][i]), _ptr(want["V"][i]), want["Y"].shape[2], want["U"].shape[2], bits,
                                     float(fades[i][0]), float(fades[i][1]))
    return want


@functools.lru_cache(maxsize=None)
def oracle_results(w, h, bits, placement, ratio):
    """what the oracle makes of a case's clip: {"scan" (9, 2), "records" (9, 33), "fades" (9, 2), "erased" {"Y", "U", "V"}}.  Read-only."""
    W, H, X, Y0, _ = geometry(w, h, placement)
    clip = tiny_clip(w, h, bits, placement)
    Y = clip["Y"]
    lo = oracle_logo(w, h, placement)
    d, t, b = oracle_eval_logos(lo, ratio)
    scan = oracle_scan([d], Y, bits, W, H)[:, 0]
    rec = np.zeros(N_FRAMES * 33, np.float32)
    oracle().lib.orc_analyze_frames(d, t, b, _ptr(Y), Y.strides[0], Y.shape[2], bits, N_FRAMES, _ptr(rec))
    rec = rec.reshape(N_FRAMES, 33)
    fades = oracle_fades(rec)
    out = dict(scan=scan, records=rec, fades=fades, erased=oracle_erase(lo, clip, bits, fades))
    for v in (scan, rec, fades, *out["erased"].values()):
        v.setflags(write=False)
    return out


def same_bytes_or_nan(got, want):
    """the rule for records: identical bytes wherever the oracle's value is not NaN, NaN (any payload) wherever it is"""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.isnan(got[nan]).all() and got[~nan].tobytes() == want[~nan].tobytes())


def assert_records(got, want, what):
    if same_bytes_or_nan(got, want):
        return
    g, w = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    nan = np.isnan(w)
    bad = np.flatnonzero(np.where(nan, ~np.isnan(g), g.view(np.uint32) != w.view(np.uint32)))
    i = int(bad[0])
    raise AssertionError("%s: %d of %d values differ from the oracle's; the first at %d: %r (%#010x) against %r (%#010x)"
                         % (what, bad.size, w.size, i, float(g[i]), int(g.view(np.uint32)[i]), float(w[i]), int(w.view(np.uint32)[i])))


# ---- placement (b): one allocation, guard containers around every plane --------------------------------------------------------------
class GuardedClip:
    """A clip laid out in ONE flat buffer of containers: GUARD containers, the Y planes of all frames (tight: pitch == width, frame after
    frame), GUARD, the U planes, GUARD, the V planes, GUARD.  A stray access of a kernel around a rectangle that is flush with a plane's
    first or last sample lands in memory the test owns, and shows: guards() must come back as they were."""

    def __init__(self, clip, fill):
        self.dt = clip["Y"].dtype
        self.shapes = {k: clip[k].shape for k in "YUV"}
        self.off, self.spans = {}, []
        pos = 0
        for k in "YUV":
            self.spans.append((pos, pos + GUARD))
            pos += GUARD
            self.off[k] = pos
            pos += int(np.prod(self.shapes[k]))
        self.spans.append((pos, pos + GUARD))
        self.size = pos + GUARD
        self.fill = fill
        self.flat = np.full(self.size, fill, self.dt)
        for k in "YUV":
            self.plane(k)[...] = clip[k]

    def plane(self, k, flat=None):
        a = self.flat if flat is None else flat
        n = int(np.prod(self.shapes[k]))
        return a[self.off[k]:self.off[k] + n].reshape(self.shapes[k])

    def guards_intact(self, flat):
        return all(bool((flat[a:b] == self.fill).all()) for a, b in self.spans)
