"""Numpy restatement of the cadence renderer on decoder surfaces ("surfaces in kind"), written from the rule and
not from the C++ code: de-interleave U and V, shift the containers to samples, apply the planar sample rule (kfm_render_ref) per plane,
shift back and re-interleave -- and take every copied row (all rows of a WEAVE, the kept rows of a BOB) verbatim from the source, low
bits included.  Checker side only."""
import numpy as np

import kfm_render_ref as R


def shift_of(bits, msb):
    return 16 - bits if msb else 0


def split_planes(planes, interleaved):
    """(Y, U, V) container planes [n, h, w] / [n, h/2, w/2] of a surface's tight planes: (Y, UV [n, h/2, w]) when interleaved"""
    if not interleaved:
        return tuple(planes)
    Y, UV = planes[0], planes[1]
    return Y, UV[:, :, 0::2], UV[:, :, 1::2]


def join_planes(yuv, interleaved):
    if not interleaved:
        return tuple(yuv)
    Y, U, V = yuv
    UV = np.empty(U.shape[:2] + (2 * U.shape[2],), U.dtype)
    UV[:, :, 0::2], UV[:, :, 1::2] = U, V
    return Y, UV


def copied_rows(entry, clip_first):
    """[(row parity, batch-local source frame)] of the rows an output frame takes as stored"""
    kind, top, bottom = int(entry[0]), int(entry[1]) - clip_first, int(entry[2]) - clip_first
    if kind == R.WEAVE:
        return [(0, top), (1, bottom)]
    return [(0, top)] if kind == R.BOB_TOP else [(1, top)]


def render_surfaces_ref(planes, plan, thresh, bits, interleaved, msb, clip_first=0, clip_frames=None):
    """The destination's tight planes -- (Y, UV) [nout, ...] interleaved, (Y, U, V) planar -- of the plan over the source's tight planes
    (containers as stored).  thresh counts samples"""
    s = shift_of(bits, msb)
    src = split_planes(planes, interleaved)
    if s and thresh >= 0:
        thresh = min(thresh, (1 << bits) - 1)
    samples = tuple(p >> s for p in src)
    out = [np.ascontiguousarray(p << s).astype(src[0].dtype) for p in R.render_ref(samples, plan, thresh, clip_first, clip_frames)]
    for k, e in enumerate(plan):
        for parity, frame in copied_rows(e, clip_first):
            for o, p in zip(out, src):
                o[k, parity::2] = p[frame, parity::2]
    return join_planes(out, interleaved)


def interpolated_rows(entry):
    """the row parity an output frame interpolates, or None for a WEAVE"""
    kind = int(entry[0])
    return None if kind == R.WEAVE else 1 if kind == R.BOB_TOP else 0
