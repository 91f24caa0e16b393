"""Numpy restatement of the cadence renderer, written from its specification and not from the C++ code: the render
plan that goes with the durations file, and the sample rule of woven and bob-deinterlaced output frames.  Checker side only."""
import numpy as np

WEAVE, BOB_TOP, BOB_BOTTOM = 0, 1, 2
CAD_60I, CAD_24P, CAD_30P = 0, 1, 2
RENDER_FRAME = np.dtype([("kind", np.int32), ("top", np.int32), ("bottom", np.int32), ("ticks", np.int32)])


def render_plan_ref(cadence, phase):
    """[(kind, top, bottom, ticks)] per output frame, absolute source frame numbers"""
    cad, ph = [int(v) for v in cadence], [int(v) for v in phase]
    n, N, out = 0, len(cad), []
    while n < N:
        if n + 5 <= N and all(cad[n + k] == CAD_24P and ph[n + k] == k for k in range(5)):
            out += [(WEAVE, n, n, 2), (WEAVE, n + 1, n + 1, 3), (WEAVE, n + 3, n + 2, 2), (WEAVE, n + 4, n + 4, 3)]
            n += 5
            continue
        if cad[n] == CAD_60I:
            out += [(BOB_TOP, n, n, 1), (BOB_BOTTOM, n, n, 1)]
        else:
            out.append((WEAVE, n, n, 2))
        n += 1
    return out


def plan_array(entries):
    return np.array([tuple(e) for e in entries], RENDER_FRAME).reshape(-1)


def _bob_plane(P, n, missing_parity, other, thresh):
    """plane n of the clip P [frames, h, w] with rows of `missing_parity` interpolated; other: the frame of the second temporal neighbour"""
    h = P.shape[1]
    cur = P[n].astype(np.int64)
    out = cur.copy()
    for y in range(missing_parity, h, 2):
        up = cur[y - 1] if y - 1 >= 0 else cur[y + 1]
        dn = cur[y + 1] if y + 1 < h else cur[y - 1]
        row = (up + dn + 1) >> 1
        if thresh >= 0:
            a, b = P[other, y].astype(np.int64), cur[y]
            row = np.where(np.abs(a - b) <= thresh, (a + b + 1) >> 1, row)
        out[y] = row
    return out.astype(P.dtype)


def render_frame_ref(planes, entry, clip_first, clip_frames, thresh):
    """One output frame: planes = (Y, U, V) arrays [frames, h, w] that hold clip frames clip_first ..; entry = (kind, top, bottom, ...) in
    absolute frame numbers.  Samples are the containers as stored."""
    kind, top, bottom = int(entry[0]), int(entry[1]), int(entry[2])
    out = []
    for P in planes:
        if kind == WEAVE:
            f = P[top - clip_first].copy()
            f[1::2] = P[bottom - clip_first, 1::2]
        elif kind == BOB_TOP:
            n = top
            other = n - 1 if n >= 1 else n                   # the bottom field before the kept top field; none at the clip's start
            f = _bob_plane(P, n - clip_first, 1, other - clip_first, thresh)
        else:
            n = top
            other = n + 1 if n + 1 < clip_frames else n      # the top field after the kept bottom field; none at the clip's end
            f = _bob_plane(P, n - clip_first, 0, other - clip_first, thresh)
        out.append(f)
    return out


def render_ref(planes, plan, thresh, clip_first=0, clip_frames=None):
    """(Y, U, V) [nout, h, w] of the plan over the tight planes of a clip (or of the batch that starts at clip_first)"""
    if clip_frames is None:
        clip_frames = clip_first + planes[0].shape[0]
    frames = [render_frame_ref(planes, e, clip_first, clip_frames, thresh) for e in plan]
    return tuple(np.stack([f[k] for f in frames]) for k in range(3))
