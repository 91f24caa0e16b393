"""Numpy restatement of the cadence renderer's edge-directed, motion-adaptive bob ("the adaptive rule"), written
from its specification and not from the kernel.  The plan, the weave and the kept rows are kfm_render_ref's.  Beside the pictures it
counts, per plane, the direction each interpolated pixel took (-2..2) and the outcome of its clamp (upper, lower, none).  Checker side
only."""
import numpy as np

import kfm_render_ref as R

DIRECTIONS = (-2, -1, 0, 1, 2)
CLAMPS = ("upper", "lower", "none")


def adaptive_row(C, P, N, A, B, y):
    """(the missing row y, the direction per pixel, the clamp outcome per pixel: 0 upper, 1 lower, 2 none); C, P, N, A, B: planes [h, w]"""
    h, w = C.shape
    y1m = y - 1 if y - 1 >= 0 else y + 1
    y1p = y + 1 if y + 1 < h else y - 1
    y2m = y - 2 if y - 2 >= 0 else y
    y2p = y + 2 if y + 2 < h else y
    i64 = lambda a: a.astype(np.int64)
    U, D = i64(C[y1m]), i64(C[y1p])
    x = np.arange(w)
    X = lambda k: np.clip(x + k, 0, w - 1)
    c, e = U, D
    a0, b0 = i64(A[y]), i64(B[y])
    d = (a0 + b0) >> 1
    t0 = np.abs(a0 - b0)
    t1 = (np.abs(i64(P[y1m]) - c) + np.abs(i64(P[y1p]) - e)) >> 1
    t2 = (np.abs(i64(N[y1m]) - c) + np.abs(i64(N[y1p]) - e)) >> 1
    diff = np.maximum(np.maximum(t0 >> 1, t1), t2)

    pred = (c + e) >> 1
    score = np.abs(U[X(-1)] - D[X(-1)]) + np.abs(c - e) + np.abs(U[X(1)] - D[X(1)]) - 1
    direction = np.zeros(w, np.int64)
    for sgn in (-1, 1):
        alive = np.ones(w, bool)                                     # +-2 is tried only where +-1 improved
        for j in (sgn, 2 * sgn):
            s = np.abs(U[X(j - 1)] - D[X(-j - 1)]) + np.abs(U[X(j)] - D[X(-j)]) + np.abs(U[X(j + 1)] - D[X(-j + 1)])
            take = alive & (s < score)
            score = np.where(take, s, score)
            pred = np.where(take, (U[X(j)] + D[X(-j)]) >> 1, pred)
            direction = np.where(take, j, direction)
            alive = take

    b = (i64(A[y2m]) + i64(B[y2m])) >> 1
    f = (i64(A[y2p]) + i64(B[y2p])) >> 1
    mx = np.maximum(np.maximum(d - e, d - c), np.minimum(b - c, f - e))
    mn = np.minimum(np.minimum(d - e, d - c), np.maximum(b - c, f - e))
    diff = np.maximum(np.maximum(diff, mn), -mx)

    upper, lower = pred > d + diff, pred < d - diff
    out = np.where(upper, d + diff, np.where(lower, d - diff, pred))
    return out, direction, np.where(upper, 0, np.where(lower, 1, 2))


def _bob_plane(Pl, n, kind, lo, hi, dirs, clamps):
    """plane n of the batch Pl [frames, h, w] with the rows of the missing parity interpolated; lo / hi: the batch-local frames n - 1 and
    n + 1 (n itself at the clip's ends)"""
    C, P, N = Pl[n], Pl[lo], Pl[hi]
    A, B = (P, C) if kind == R.BOB_TOP else (C, N)
    out = C.copy()
    for y in range(1 if kind == R.BOB_TOP else 0, C.shape[0], 2):
        row, dr, cl = adaptive_row(C, P, N, A, B, y)
        assert row.min() >= 0 and row.max() <= np.iinfo(Pl.dtype).max, "the rule left the container's range"
        out[y] = row.astype(Pl.dtype)
        for k, j in enumerate(DIRECTIONS):
            dirs[k] += int((dr == j).sum())
        for k in range(3):
            clamps[k] += int((cl == k).sum())
    return out


def render_adaptive_ref(planes, plan, clip_first=0, clip_frames=None):
    """((Y, U, V) [nout, h, w], counts) of the plan over the tight planes of a clip (or of the batch that starts at clip_first);
    counts[plane] = {"dir": [pixels that took -2, -1, 0, 1, 2], "clamp": [upper, lower, none]}"""
    if clip_frames is None:
        clip_frames = clip_first + planes[0].shape[0]
    counts = [{"dir": [0] * 5, "clamp": [0] * 3} for _ in range(3)]
    frames = []
    for e in plan:
        kind, n = int(e[0]), int(e[1])
        if kind == R.WEAVE:
            frames.append(R.render_frame_ref(planes, e, clip_first, clip_frames, -1))
            continue
        lo = n - 1 if n >= 1 else n
        hi = n + 1 if n + 1 < clip_frames else n
        assert clip_first <= lo and hi < clip_first + planes[0].shape[0], "a bob entry needs both neighbours inside the batch"
        frames.append([_bob_plane(Pl, n - clip_first, kind, lo - clip_first, hi - clip_first, counts[k]["dir"], counts[k]["clamp"])
                       for k, Pl in enumerate(planes)])
    return tuple(np.stack([f[k] for f in frames]) for k in range(3)), counts
