"""Named lists of candidate logos that differ in size and position, and builders that turn one list into the forms the tests need:
the numpy planes, the oracle's handles (deinterlaced and masked, what LogoFrame evaluates), `.lgd` files and amatsukaze_amd.Logo objects.

LogoFrame scores a list of `.lgd` files of different channels against one clip (CMAnalyze.hpp:291-299, LogoScan.hpp:1521-1836); every
file has its own width, height and position.  Lists whose logos share one rectangle cannot tell per-logo state apart -- a table base, a
band count, a column offset or an LDS plane taken from the wrong logo -- so the scan tests take their lists from here.

A plain helper module (no fixtures): tests import what they need.  Checker side only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import amt_synth as S
from amtlib import _ptr

MASKRATIO = 0.35

# Every entry is (w, h, imgx, imgy).  Heights are even: amt_synth.make_logo averages 2 x 2 blocks for the chroma planes.
#
# SMALL_MIXED, in a 352 x 240 frame; the clip is the one of test_gpu_parity.SMALL (logo A blended in):
#   A  the clip's own logo
#   B  tall and narrow, origin % 4 == 2, many short bands
#   C  w % 4 == 2, on the first row of the frame, few bands
#   D  wider than a wave's 64 lanes x 4 columns, ends on the last row and the last column
#   E  exactly the bottom-right corner, overlaps D
SMALL_FRAME = (352, 240)
LOGO_A = (96, 48, 224, 18)
LOGO_B = (36, 100, 6, 120)
LOGO_C = (130, 20, 110, 0)
LOGO_D = (322, 40, 30, 200)
LOGO_E = (96, 48, 256, 192)
SMALL_MIXED = [LOGO_A, LOGO_B, LOGO_C, LOGO_D, LOGO_E]

# WIDE_MIXED, in an 800 x 96 frame (the frame of w680_column_bands in test_gpu_eval_shapes.py): a logo whose bands the generic
# kernel stages by columns next to two that stage whole rows
WIDE_FRAME = (800, 96)
WIDE_MIXED = [(680, 24, 60, 30), (36, 60, 2, 4), (130, 20, 400, 70)]

# w < 6: the pair kernel's tiles are four columns wide, the whole list goes to the generic kernel.  No window fits (LogoScan.hpp:184-185
# walks x in [2, w - 2)): no mask pixel is ever evaluated and the records are 0 / 0.
TINY = (4, 6, 100, 100)

# what make_logo draws for an entry: (seed, strength).  A and the 680-wide logo are make_logo's default, the logo test_gpu_parity.make_case
# blends into its clips.
_DRAW = {
    LOGO_A: (0x10600001, 1.0), LOGO_B: (0x10600012, 0.8), LOGO_C: (0x10600013, 0.9), LOGO_D: (0x10600014, 0.7), LOGO_E: (0x10600015, 0.6),
    WIDE_MIXED[0]: (0x10600001, 1.0), WIDE_MIXED[1]: (0x10600022, 0.8), WIDE_MIXED[2]: (0x10600023, 0.9),
    TINY: (0x10600031, 1.0),
}

_planes_cache: dict = {}


def logo_planes(entry):
    """(data, alphaY, alphaUV) of amt_synth.make_logo for the entry; the arrays are shared and read-only"""
    if entry not in _planes_cache:
        seed, strength = _DRAW.get(entry, (0x10600040 + entry[0] * 131 + entry[1], 1.0))
        got = S.make_logo(entry[0], entry[1], seed=seed, strength=strength)
        for a in got:
            a.setflags(write=False)
        _planes_cache[entry] = got
    return _planes_cache[entry]


def logo_data(entry):
    return logo_planes(entry)[0]


class Built:
    """One list in every form.  `data`, `raw` (the oracle's LogoData handles), `evals` (their deinterlaced, masked evaluation logos:
    what orc_logoframe_scan takes), `paths` (.lgd files) and `logos` (amatsukaze_amd.Logo) are parallel lists; the forms that were not
    asked for are None."""

    def __init__(self, entries, frame, data, raw, evals, paths, logos):
        self.entries, self.frame, self.data, self.raw, self.evals, self.paths, self.logos = entries, frame, data, raw, evals, paths, logos


def build(entries, frame, orc=None, ctx=None, lgd_dir=None, maskratio=MASKRATIO, data=None, frames=None):
    """`data[i]` replaces the planes of entry i (a test that plants a coefficient); `frames[i]` the frame size entry i was made for"""
    datas = [np.ascontiguousarray(data[i] if data and data.get(i) is not None else logo_data(e), np.float32) for i, e in enumerate(entries)]
    sizes = [frames.get(i, frame) if frames else frame for i in range(len(entries))]
    raw = evals = paths = logos = None
    if orc is not None:
        raw = [orc.make_logo(d, e[0], e[1], fw, fh, e[2], e[3]) for d, e, (fw, fh) in zip(datas, entries, sizes)]
        evals = [oracle_eval_logo(orc, h, maskratio) for h in raw]
        if lgd_dir is not None:
            paths = []
            for i, h in enumerate(raw):
                p = str(lgd_dir / f"logo{i}_{entries[i][0]}x{entries[i][1]}.lgd")
                assert orc.lib.orc_logo_save(h, p.encode(), b"logo%d" % i, 1000 + i) == 1
                paths.append(p)
    if ctx is not None:
        from amatsukaze_amd import Logo
        logos = [Logo.from_planes(ctx, d, e[0], e[1], fw, fh, e[2], e[3]) for d, e, (fw, fh) in zip(datas, entries, sizes)]
    return Built(list(entries), frame, datas, raw, evals, paths, logos)


def oracle_eval_logo(orc, handle, maskratio=MASKRATIO):
    """the logo LogoFrame evaluates: deinterlaced, CreateLogoMask applied (LogoScan.hpp:1615-1620)"""
    d = orc.lib.orc_logo_deint(handle)
    orc.lib.orc_logo_create_mask(d, maskratio, 1)
    return d


def oracle_scan(orc, evals, Y, bits, frame):
    """orc_logoframe_scan over the list -> [frames][logos][2]; None in `evals` is a slot whose file could not be read (a null handle)"""
    n, nl = int(Y.shape[0]), len(evals)
    out = np.zeros(n * nl * 2, np.float32)
    orc.lib.orc_logoframe_scan((C.c_void_p * nl)(*evals), nl, _ptr(Y), Y.strides[0], Y.shape[2], bits, frame[0], frame[1], n, _ptr(out))
    return out.reshape(n, nl, 2)


def oracle_decide(orc, want, ncand, logo_index, fps=(30000, 1001)):
    """(best logo, ratio as float32, logoframe text) of the oracle from records [frames][logos][2]"""
    n, nl = want.shape[0], want.shape[1]
    flat = np.ascontiguousarray(want.reshape(-1), np.float32)
    best, ratio = C.c_int(), C.c_float()
    orc.lib.orc_logoframe_select(_ptr(flat), n, nl, ncand, C.byref(best), C.byref(ratio))
    buf = C.create_string_buffer(1 << 16)
    ln = orc.lib.orc_logoframe_write_result(_ptr(flat), n, nl, best.value if logo_index < 0 else logo_index, fps[0], fps[1], buf, len(buf))
    assert ln >= 0
    return best.value, np.float32(ratio.value), buf.raw[:ln]


def write_mask_positions(orc, eval_logo, path):
    """The mask pixels CorrelationScore visits (LogoScan.hpp:295-297: rows and columns [2, size - 2)) of a masked oracle logo, as the file
    tests/cpp/eval_tiles_test.cpp and tile_cut_test.cpp read: int32 {count, w, h}, then uint32 (y << 16 | x) in raster order.
    Returns (count, w, h)."""
    info = orc.logo_info(eval_logo)
    w, h = int(info[0]), int(info[1])
    mask = orc.logo_arrays(eval_logo)[1].reshape(h, w)
    ys, xs = np.nonzero(mask[2:h - 2, 2:w - 2])
    pos = ((ys + 2).astype(np.uint32) << 16) | (xs + 2).astype(np.uint32)
    with open(path, "wb") as f:
        np.array([len(pos), w, h], np.int32).tofile(f)
        pos.astype(np.uint32).tofile(f)
    return len(pos), w, h


# (entry, mask ratio) of every geometry the mixed scans run, plus the smallest logo the tile plans take -- 6 x 6 with every pixel in the
# mask: the four whose window fits -- and a sparse mask on a w % 4 == 2 logo
REPLAY_CASES = [(e, MASKRATIO) for e in SMALL_MIXED + WIDE_MIXED] + [((6, 6, 0, 0), 1.0), (LOGO_C, 0.02)]
REPLAY_IDS = ["%dx%d@%d,%d-%g" % (e + (r,)) for e, r in REPLAY_CASES]
