"""Three small frames placed gigabytes apart in ONE allocation, and deliberately wrong restatements ("mutants") of how a kernel might
form a frame's address, in numpy and address arithmetic only (the style of tests/plane_edge_clips.py).

Frame n of a plane lies at byte `base + n * S` of a flat allocation of A bytes.  Two layouts share the allocation (and frame 0): L31 with
S = 2^31 + D1 (the byte products n * S cross 2^31 and 2^32) and L32 with S = 2^32 + D2 (n * S / 2 crosses 2^31 and 2^32 for the 16-bit
launchers that count in samples).  Every plane (or decoder surface) has a slot of SLOT bytes; slot k's frame 0 starts at B + k * SLOT.

A mutant acts on the frame offset p = n * S_u in the unit u the kernel counts in (bytes, or samples = S / 2 where a launcher divides the
stride): `u32` keeps p mod 2^32, `s32` sign-extends that, `stride_u32` / `stride_s32` truncate the STRIDE and multiply in 64 bits.  At
every address a mutant forms for n > 0 the allocation holds a decoy -- another picture of the same geometry -- so a kernel that is wrong
in a modelled way reads or writes the test's own memory and shows wrong bytes; it never leaves the allocation.  B = 4 GiB is what keeps
the sign-extended (negative) offsets inside.  tests/test_far_stride_layout_host.py pins all of that without a GPU.

The pictures are the SMALL case of test_gpu_parity.py (352 x 240, a 96 x 48 logo at (224, 18)) at 8 bits and at 10 bits in 16-bit
containers, planar LSB and as NV12 / P010 surfaces (Y and UV in one surface: strideY == strideUV == S).  Two more groups of slots serve
the cadence renderer, which wants its two batches one behind the other: a second L31 batch (RD) and a batch of near frames (NEAR).  `Refs` states every operation
of tests/test_gpu_far_strides.py with the CPU oracle and the numpy references; both test files take their expected values from it."""
from __future__ import annotations

import ctypes as C
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import amt_synth as S
import audio_clips as AC
import copy_cases as CC
import frame_stats_oracle as FS
import kfm_render_adaptive_ref as RA
import kfm_render_adaptive_surfaces_ref as RAS
import kfm_render_ref as R
import kfm_render_surfaces_ref as RS
import logofind_ref as LF
import surface_clips as SC
import surface_erase_ref as SE
from amtlib import Oracle, _ptr

GiB, MiB = 1 << 30, 1 << 20
M32 = (1 << 32) - 1

# ---------------------------------------------------------------------------------------------------------------- layout
N = 3
B = 4 * GiB                            # frame 0 of slot 0
D1, D2 = 5 * MiB, 15 * MiB             # multiples of 256 bytes, larger than all the slots together
SLOT = 256 * 1024                      # bytes of a slot: the largest window (a P010 surface, 253 440 bytes) and a 4 KiB guard band
LAYOUTS = {"L31": (1 << 31) + D1, "L32": (1 << 32) + D2}
STRIDES = dict(LAYOUTS, near=SLOT)     # "near": frames one slot apart, for the other side of an operation that cannot have both sides far
MAIN = ("p8Y", "p8U", "p8V", "p10Y", "p10U", "p10V", "nv12", "p010", "prev8", "prev10", "dstY", "dstU", "dstV", "dstS", "prevP010", "spare")
# The cadence renderer refuses a destination whose byte range (first byte of frame 0 to last byte of the last frame) touches the
# source's.  Two L31 batches fit one behind the other -- the second, RD, starts behind frame 2 of the first --; two L32 batches would
# need 16 GiB.  An L32 batch is therefore rendered to and from a batch of near frames in front of every far one.
RD = B + (1 << 32) + 25 * MiB
NEAR = 40 * MiB
REGIONS = {k: (B + i * SLOT, ("L31", "L32")) for i, k in enumerate(MAIN)}
REGIONS.update({k: (RD + i * SLOT, ("L31",)) for i, k in enumerate(("rdY", "rdU", "rdV", "rdS"))})
REGIONS.update({k: (NEAR + i * MiB, ("near",)) for i, k in enumerate(("nearY", "nearU", "nearV", "nearS"))})
SLOT_NAMES = tuple(REGIONS)
A = RD + (N - 1) * LAYOUTS["L31"] + 4 * SLOT                  # 12 GiB + 36 MiB
CAP = 13 * GiB
GUARD = 4096

MUTANTS = ("u32", "s32", "stride_u32", "stride_s32")
UNITS = (1, 2)                         # bytes of the unit a kernel counts frame offsets in: bytes, or 16-bit samples
# frame 2 of L32 would lie at B - 2^33 + 2 * D2 < 0: keeping that inside needs B >= 8 GiB and an allocation of 16 GiB, above the cap.
# (In L31 the sample stride is below 2^31, so the mutant does not apply there either.)
DROPPED = {("stride_s32", 2): "frame 2 of L32 would lie 4 GiB in front of the allocation"}

# modelled, in bounds, but equal to the true address in both layouts: a sample stride only loses bits from 2^32 samples = 8 GiB on, and
# three frames that far apart do not fit under the cap
INERT = {("stride_u32", 2)}


def _sext32(v):
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def true_offset(n, S_bytes):
    return n * S_bytes


def mutant_offset(name, n, S_bytes, unit):
    """byte offset of frame n from frame 0 as the wrong kernel forms it"""
    assert S_bytes % unit == 0
    Su = S_bytes // unit
    if name == "u32":
        p = (n * Su) & M32
    elif name == "s32":
        p = _sext32(n * Su)
    elif name == "stride_u32":
        p = n * (Su & M32)
    elif name == "stride_s32":
        p = n * _sext32(Su)
    else:
        raise ValueError(name)
    return p * unit


def modelled():
    """[(mutant, unit)] of the pairs the layout keeps in bounds"""
    return [(m, u) for m in MUTANTS for u in UNITS if (m, u) not in DROPPED]


def _decoys():
    seen = {}
    for lay, Sb in STRIDES.items():
        for m, u in modelled():
            for n in range(1, N):
                off = mutant_offset(m, n, Sb, u)
                if off != true_offset(n, Sb):
                    assert seen.setdefault(off, (n, lay)) == (n, lay)
    return tuple((off, n, lay) for off, (n, lay) in sorted(seen.items()))


DECOYS = _decoys()                     # ((byte offset from frame 0, the frame number a mutant means there, in which layout), ...)


def slot_base(slot):
    return REGIONS[slot][0]


def slot_layouts(slot):
    return REGIONS[slot][1]


def true_windows(slot, layout):
    """absolute byte address of frames 0..N-1"""
    assert layout in slot_layouts(slot), (slot, layout)
    return [slot_base(slot) + true_offset(n, STRIDES[layout]) for n in range(N)]


def decoy_windows(slot):
    """[(index into DECOYS, absolute byte address)] of the decoys a slot holds: those of its layouts"""
    return [(w, slot_base(slot) + off) for w, (off, _, lay) in enumerate(DECOYS) if lay in slot_layouts(slot)]


def all_windows():
    """[(first byte, last byte + 1, slot, "true" / "decoy")] of every window of every slot"""
    out = []
    for slot in SLOT_NAMES:
        ext = window_extent(slot)
        firsts = {a for lay in slot_layouts(slot) for a in true_windows(slot, lay)}
        out += [(a, a + ext, slot, "true") for a in sorted(firsts)]
        out += [(a, a + ext, slot, "decoy") for _, a in decoy_windows(slot)]
    return out


# ---------------------------------------------------------------------------------------------------------------- audio
# The PCM of three video frames in the allocation seen as ONE int16 tensor that starts at byte PCM_BASE: their first element is
# PCM_ELEM >= 2^31 (byte 2^32 of the tensor).  Wrapped, the element offset is negative and the byte offset small: decoy PCM lies at both.
SAMPLE_RATE, CHANNELS, FPS = 48000, 2, (30000, 1001)
PCM_BASE = B
PCM_GAP = 20 * MiB                      # what the byte offset 2^32 + PCM_GAP keeps mod 2^32: free between the video windows
AUDIO_FIRST_FRAME = 700000
PCM_START = AC.frame_start(AUDIO_FIRST_FRAME, SAMPLE_RATE, *FPS)                       # sample-frame of the first video frame
PCM_ELEM = ((1 << 32) + PCM_GAP) // 2                                                  # element of the tensor that holds it
PCM_FIRST = PCM_START - PCM_ELEM // CHANNELS                                           # sample-frame of the tensor's element 0
PCM_FRAMES = AC.frame_start(AUDIO_FIRST_FRAME + N, SAMPLE_RATE, *FPS) - PCM_START      # sample-frames of the three video frames
PCM_BYTES = PCM_FRAMES * CHANNELS * 2
PCM_NUMEL = PCM_ELEM + PCM_FRAMES * CHANNELS
PCM_TRUE = PCM_BASE + 2 * PCM_ELEM
PCM_DECOYS = {"elem_s32": PCM_BASE + 2 * _sext32(PCM_ELEM), "byte_u32": PCM_BASE + ((2 * PCM_ELEM) & M32)}


def pcm(seed):
    return np.random.RandomState(seed).randint(-32768, 32768, size=(PCM_FRAMES, CHANNELS)).astype(np.int16)


def audio_ref(samples):
    return AC.levels_ref_window(samples, PCM_START, SAMPLE_RATE, CHANNELS, *FPS, PCM_START + PCM_FRAMES, AUDIO_FIRST_FRAME, N)


# ---------------------------------------------------------------------------------------------------------------- pictures
W, H, LW, LH, IMGX, IMGY = 352, 240, 96, 48, 224, 18
SEED = 0x5EED0F00
THY = 12
KINDS = ("p8", "p10", "nv12", "p010")
BITS = {"p8": 8, "p10": 10, "nv12": 8, "p010": 10}
HOT = (2, IMGY + 7, IMGX + 13, 3000)             # frame, row, column, value: one sample above maxv inside the rectangle (10 bits)
FADES = np.array([[0.3, 0.8], [1.0, 1.0], [0.5, 0.0]], np.float32)
# weaves across frames, then bobs frame 1: every source frame is read, frames 0 and 2 as the temporal neighbours of frame 1 too
PLAN = R.plan_array([(R.WEAVE, 2, 1, 2), (R.BOB_TOP, 1, 1, 1), (R.BOB_BOTTOM, 1, 1, 1)])
WEAVE_TOP, WEAVE_BOTTOM = (2, 0, 1), (1, 2, 0)


@functools.lru_cache(maxsize=None)
def logo():
    return S.make_logo(LW, LH)


def _clip(n, seed, bits, start=0):
    _, alpha, alphaUV = logo()
    return S.make_clip_np(n, W, H, seed, alpha, alphaUV, IMGX, IMGY, bits=bits, period=900, fade=12, flat_every=1, start=start)


def _surf(clip, bits, msb, seed):
    return SC.to_surfaces(clip, bits, True, msb, np.random.default_rng(seed))


@functools.lru_cache(maxsize=None)
def pictures():
    """{kind: {"true": planes of N frames, "decoy": [planes of one frame per entry of DECOYS], "prev": planes of one frame}}; planes are
    {"Y", "U", "V"} arrays [frames, rows, row] -- "U" the interleaved plane and "V" None for nv12 / p010.  Read-only."""
    out = {}
    for kind, bits in (("p8", 8), ("p10", 10)):
        out[kind] = {"true": _clip(N, SEED + bits, bits),
                     "decoy": [_clip(1, SEED + bits + 0x100 * (w + 1), bits, start=n) for w, (_, n, _lay) in enumerate(DECOYS)],
                     "prev": _clip(1, SEED + bits + 0x77, bits, start=9)}
    for kind, src, msb in (("nv12", "p8", False), ("p010", "p10", True)):
        bits = BITS[kind]
        out[kind] = {"true": _surf(out[src]["true"], bits, msb, SEED + 1),
                     "decoy": [_surf(d, bits, msb, SEED + 2 + w) for w, d in enumerate(out[src]["decoy"])],
                     "prev": _surf(out[src]["prev"], bits, msb, SEED + 99)}
    for k in out.values():
        for planes in [k["true"], k["prev"]] + k["decoy"]:
            for a in planes.values():
                if a is not None:
                    a.setflags(write=False)
    return out


def swapped(kind, w):
    """the true frames of a kind with decoy w in the place of the frame a mutant means there"""
    p = pictures()[kind]
    n = DECOYS[w][1]
    out = {}
    for k, a in p["true"].items():
        if a is None:
            out[k] = None
            continue
        a = a.copy()
        a[n] = p["decoy"][w][k][0]
        out[k] = a
    return out


def with_hot_sample(planes):
    f, y, x, v = HOT
    out = {k: a.copy() for k, a in planes.items()}
    out["Y"][f, y, x] = v
    return out


def plane_bytes(a):
    """the bytes of one frame of a plane as they lie in its window"""
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def surface_bytes(planes, f):
    """one decoder surface: its Y plane and, right behind it, its UV plane"""
    return np.concatenate([plane_bytes(planes["Y"][f]), plane_bytes(planes["U"][f])])


def window_extent(slot):
    """bytes a slot's frame windows hold (the destinations: the largest picture they take)"""
    p = pictures()
    if slot in ("p8Y", "p8U", "p8V", "p10Y", "p10U", "p10V"):
        return plane_bytes(p[slot[:-1]]["true"][slot[-1]][0]).size
    if slot == "nv12":
        return surface_bytes(p["nv12"]["true"], 0).size
    if slot == "prev8":
        return plane_bytes(p["p8"]["prev"]["Y"][0]).size
    if slot == "spare":
        return SLOT - 2 * GUARD
    if slot[-1] in "UV":
        return plane_bytes(p["p10"]["true"]["U"][0]).size
    if slot[-1] == "Y" or slot == "prev10":
        return plane_bytes(p["p10"]["true"]["Y"][0]).size
    return surface_bytes(p["p010"]["true"], 0).size          # p010, prevP010, dstS, rdS, nearS


# ---------------------------------------------------------------------------------------------------------------- references
def _tight(a):
    return np.ascontiguousarray(a)


class Refs:
    """every operation of test_gpu_far_strides.py on three frames, with the CPU oracle and the numpy references"""

    def __init__(self):
        self.orc = orc = Oracle()
        self.data = logo()[0]
        self.big = self.data.copy()
        self.big.reshape(-1)[LW * 2 + 5] = 1e31          # keeps the scan off the pair kernel (test_logoframe_scan_kernel_choice)
        self.lo = orc.make_logo(self.data, LW, LH, W, H, IMGX, IMGY)
        self.lo_big = orc.make_logo(self.big, LW, LH, W, H, IMGX, IMGY)
        self.eval = self._eval_logos(self.lo)
        self.eval_big = self._eval_logos(self.lo_big)

    def _eval_logos(self, lo, maskratio=0.35):
        out = []
        for h in (self.orc.lib.orc_logo_deint(lo), self.orc.lib.orc_logo_field(lo, 0), self.orc.lib.orc_logo_field(lo, 1)):
            self.orc.lib.orc_logo_create_mask(h, maskratio, 1)
            out.append(h)
        return out

    # -- logo passes
    def analyze(self, planes, bits):
        Y = _tight(planes["Y"])
        want = np.zeros(Y.shape[0] * 33, np.float32)
        d, t, b = self.eval
        self.orc.lib.orc_analyze_frames(d, t, b, _ptr(Y), Y.strides[0], Y.shape[2], bits, Y.shape[0], _ptr(want))
        return want.reshape(-1, 33)

    def scan(self, planes, bits, generic=False):
        Y = _tight(planes["Y"])
        want = np.zeros(Y.shape[0] * 2, np.float32)
        d = (self.eval_big if generic else self.eval)[0]
        self.orc.lib.orc_logoframe_scan((C.c_void_p * 1)(d), 1, _ptr(Y), Y.strides[0], Y.shape[2], bits, W, H, Y.shape[0], _ptr(want))
        return want.reshape(-1, 1, 2)

    def erase(self, planes, bits, fades=FADES):
        return SE.oracle_planes(self.orc, self.lo, planes, bits, fades)

    def erase_surfaces(self, surf, bits, msb, fades=FADES):
        return SE.expected_surfaces(self.orc, self.lo, surf, W, H, bits, True, msb, (IMGX, IMGY, LW, LH), fades, True)

    def logoscan(self, planes):
        """(AddFrame's verdicts, the oracle's sums [pixels, 5]) of 8-bit frames"""
        so = self.orc.lib.orc_scan_create(LW, LH, 1, 1, THY)
        Y, U, V = (_tight(planes[k]) for k in "YUV")
        valid = [self.orc.lib.orc_scan_add_frame_u8(so, Y[i, IMGY:, IMGX:].ctypes.data, U[i, IMGY // 2:, IMGX // 2:].ctypes.data,
                                                    V[i, IMGY // 2:, IMGX // 2:].ctypes.data, Y.shape[2], U.shape[2]) for i in range(Y.shape[0])]
        npx = LW * LH + 2 * (LW // 2) * (LH // 2)
        osum = np.zeros(npx * 5)
        self.orc.lib.orc_scan_sums(so, _ptr(osum))
        self.orc.lib.orc_scan_free(so)
        return np.array(valid, np.int32), osum.reshape(npx, 5)

    def scanlogo_lgd(self, planes, rounds, path):
        """the .lgd of ScanLogo over the batch fed `rounds` times, with a quota of every frame"""
        Y, U, V = (_tight(np.concatenate([planes[k]] * rounds)) for k in "YUV")
        nvalid, nread = C.c_int(), C.c_int()
        lo = self.orc.lib.orc_scanlogo_mt(_ptr(Y), _ptr(U), _ptr(V), Y.strides[0], U.strides[0], Y.shape[2], U.shape[2], W, H, Y.shape[0], IMGX, IMGY,
                                          LW, LH, THY, N * rounds, 1, C.byref(nvalid), None, 1, C.byref(nread))
        assert lo and nvalid.value == N * rounds, (lo, nvalid.value)
        assert self.orc.lib.orc_logo_save(lo, str(path).encode(), b"No Name", 1041) == 1
        self.orc.lib.orc_logo_free(lo)
        with open(path, "rb") as f:
            return f.read()

    # -- whole-frame passes
    @staticmethod
    def frame_stats(Y, prevY, shift=0):
        return FS.frame_metrics(np.asarray(Y) >> shift, np.asarray(prevY)[0] >> shift)

    @staticmethod
    def logofind(Y, shift=0):
        return LF.sums(np.asarray(Y) >> shift, W, H)

    @staticmethod
    def weave(planes, nv12, shift):
        return CC.weave(planes["Y"], planes["U"], planes["V"], WEAVE_TOP, WEAVE_BOTTOM, nv12, shift)

    @staticmethod
    def render(kind, planes, deint, thresh):
        """the destination's tight planes: (Y, U, V), or (Y, UV) for the surfaces"""
        bits = BITS[kind]
        if kind in ("p8", "p10"):
            src = (planes["Y"], planes["U"], planes["V"])
            return RA.render_adaptive_ref(src, PLAN)[0] if deint == "adaptive" else R.render_ref(src, PLAN, thresh)
        src, msb = (planes["Y"], planes["U"]), kind == "p010"
        if deint == "adaptive":
            return RAS.render_adaptive_surfaces_ref(src, PLAN, bits, True, msb)[0]
        return RS.render_surfaces_ref(src, PLAN, thresh, bits, True, msb)


RENDER_MODES = (("line", -1), ("line", 4), ("adaptive", -1))


def operations(refs, tmp):
    """[(name, kind, f(planes) -> list of arrays)]: what every GPU test reads of its far frames, as a function of those frames"""
    p = pictures()
    sh = {"p8": 0, "p10": 0, "nv12": 0, "p010": 6}
    ops = []
    for kind in ("p8", "p10"):
        bits = BITS[kind]
        ops.append((f"analyze-{kind}", kind, lambda pl, bits=bits: [refs.analyze(pl, bits)]))
        ops.append((f"scan_pair-{kind}", kind, lambda pl, bits=bits: [refs.scan(pl, bits)]))
        ops.append((f"scan_generic-{kind}", kind, lambda pl, bits=bits: [refs.scan(pl, bits, True)]))
        ops.append((f"erase-{kind}", kind, lambda pl, bits=bits: list(refs.erase(pl, bits).values())))
        ops.append((f"weave-{kind}", kind, lambda pl: refs.weave(pl, False, 0)))
    ops.append(("analyze_hot-p10", "p10", lambda pl: [refs.analyze(with_hot_sample(pl), 10)]))
    ops.append(("logoscan-p8", "p8", lambda pl: [refs.logoscan(pl)[1]]))          # (the verdicts are all 1: the sums tell)
    ops.append(("scanlogo_stream-p8", "p8", lambda pl: [np.frombuffer(refs.scanlogo_lgd(pl, 2, os.path.join(tmp, "far.lgd")), np.uint8)]))
    ops.append(("scanlogo_stream-nv12", "nv12",
                lambda pl: [np.frombuffer(refs.scanlogo_lgd(SC.from_surfaces(pl, W, H, 8, True, False), 2, os.path.join(tmp, "far.lgd")), np.uint8)]))
    ops.append(("extract_rect-p010", "p010", lambda pl: list(SC.crop(SC.from_surfaces(pl, W, H, 10, True, True), IMGX, IMGY, LW, LH).values())))
    ops.append(("erase_surfaces-nv12", "nv12", lambda pl: [a for a in refs.erase_surfaces(pl, 8, False).values() if a is not None]))
    ops.append(("erase_surfaces-p010", "p010", lambda pl: [a for a in refs.erase_surfaces(pl, 10, True).values() if a is not None]))
    ops.append(("weave-nv12", "nv12", lambda pl: refs.weave(pl, True, 0)))
    ops.append(("weave-p010", "p010", lambda pl: refs.weave(pl, True, 6)))
    for kind in KINDS:
        prev = p[kind]["prev"]["Y"]
        if kind != "nv12":
            ops.append((f"frame_stats-{kind}", kind, lambda pl, prev=prev, s=sh[kind]: [refs.frame_stats(pl["Y"], prev, s)]))
            ops.append((f"logofind-{kind}", kind, lambda pl, s=sh[kind]: [refs.logofind(pl["Y"], s)]))
        for deint, thresh in RENDER_MODES:
            ops.append((f"render_{deint}{thresh}-{kind}", kind, lambda pl, k=kind, d=deint, t=thresh: list(refs.render(k, pl, d, t))))
    # the row copies move the frames as they are
    ops.append(("upload_strided-p8", "p8", lambda pl: [pl["Y"]]))
    return ops
