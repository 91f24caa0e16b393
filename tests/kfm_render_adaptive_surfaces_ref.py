"""Numpy restatement of the adaptive bob on decoder surfaces ("the adaptive rule on surfaces"), written from the
rule by composing what exists and not from the kernel: de-interleave U and V (kfm_render_surfaces_ref.split_planes), shift the containers
to samples, apply the planar adaptive rule per plane (kfm_render_adaptive_ref.render_adaptive_ref), shift back, take every copied row (all
rows of a WEAVE, the kept rows of a BOB) verbatim from the source, low bits included, and re-interleave.  Checker side only."""
import numpy as np

import kfm_render_adaptive_ref as A
import kfm_render_surfaces_ref as S


def render_adaptive_surfaces_ref(planes, plan, bits, interleaved, msb, clip_first=0, clip_frames=None):
    """(the destination's tight planes -- (Y, UV) [nout, ...] interleaved, (Y, U, V) planar --, counts) of the plan over the source's
    tight planes (containers as stored); counts[k] for Y, U, V: kfm_render_adaptive_ref's directions and clamp outcomes per plane"""
    s = S.shift_of(bits, msb)
    src = S.split_planes(planes, interleaved)
    samples = tuple(np.ascontiguousarray(p >> s) for p in src)
    rendered, counts = A.render_adaptive_ref(samples, plan, clip_first, clip_frames)
    out = [np.ascontiguousarray(p << s).astype(src[0].dtype) for p in rendered]
    for k, e in enumerate(plan):
        for parity, frame in S.copied_rows(e, clip_first):
            for o, p in zip(out, src):
                o[k, parity::2] = p[frame, parity::2]
    return S.join_planes(out, interleaved), counts


def shortcut_ref(planes, plan, bits, msb):
    """what a kernel computes that walks an interleaved UV plane as ONE plane of `width` containers under the planar rule (the line
    kernel's trick): wrong here, because the rule looks sideways.  (Y, UV) of an interleaved source"""
    s = S.shift_of(bits, msb)
    Y, UV = planes
    # (the planar reference wants three planes: the UV plane twice, at its own size)
    samples = (np.ascontiguousarray(Y >> s), np.ascontiguousarray(UV >> s), np.ascontiguousarray(UV >> s))
    rendered, _ = A.render_adaptive_ref(samples, plan)
    out = [np.ascontiguousarray(p << s).astype(Y.dtype) for p in rendered[:2]]
    for k, e in enumerate(plan):
        for parity, frame in S.copied_rows(e, 0):
            for o, p in zip(out, (Y, UV)):
                o[k, parity::2] = p[frame, parity::2]
    return tuple(out)
