"""numpy restatement of the temporal noise reduction (amtgpu_temporal_nr, include/amt_gpu.h; the reference's TemporalNRFilter,
VideoFilter.hpp:156-211): vectorised over pixels, sequential over the window, every product and sum one np.float32 operation and the
factor np.float32(1) / count.  tests/test_temporal_nr_host.py holds it against tests/golden/temporal_nr_v1.npz, which the compiled
reference wrote.

Three deliberately WRONG variants show which pixels tell a right kernel from a wrong one (only counts with an inexact reciprocal whose
mean can end in .5 do: 6, 10, 12, 14 ...):
  "fma"       each step rounds once, factor * sample + sum contracted (via float64, where product and sum are exact)
  "reversed"  the window is added last frame first
  "rational"  the exact mean, rounded half up
and `stream_windows` replays the reference's onFrame / finish deque on frame numbers alone."""
import collections

import numpy as np

VARIANTS = ("ref", "fma", "reversed", "rational")


def window(t, d, clip_frames):
    """the frames of output frame t's window, in order: clamp(t + k, 0, clip_frames - 1), k = -d .. d"""
    return [min(max(t + k, 0), clip_frames - 1) for k in range(-d, d + 1)]


def stream_windows(d, clip_frames):
    """[(centre, window)] as TemporalNRFilter emits them for frames 0 .. clip_frames - 1 pushed through onFrame and then finish"""
    n = 2 * d + 1
    q, out = collections.deque(), []
    for f in range(clip_frames):
        q.append(f)
        half = (n + 1) // 2
        if len(q) < half:
            continue
        out.append((q[len(q) - half], [q[max(len(q) - n + i, 0)] for i in range(n)]))
        if len(q) >= n:
            q.popleft()
    half = n // 2
    while len(q) > half:
        out.append((q[half], [q[min(i, len(q) - 1)] for i in range(n)]))
        q.popleft()
    return out


def chroma_rows(h, interlaced):
    y = np.arange(h)
    return (((y >> 1) & ~1) | (y & 1)) if interlaced else (y >> 1)


def filter_frame(planes, t, d, threshold, bits, interlaced=False, variant="ref", win=None):
    """output frame t of the clip `planes` = (Y [n, h, w], U, V [n, h / 2, w / 2]): (Y, U, V, count [h, w]).  win: the window's frames
    (default: the clamp rule over the whole clip)"""
    assert variant in VARIANTS
    Y, U, V = planes
    n, h, w = Y.shape
    assert h % 2 == 0 and w % 2 == 0 and (not interlaced or h % 4 == 0)
    dt = Y.dtype
    win = window(t, d, n) if win is None else list(win)
    thresh = threshold << (bits - 8)
    cy, cx = chroma_rows(h, interlaced), np.arange(w) >> 1
    up = lambda P: P[cy][:, cx]                                      # a chroma plane at every luma pixel
    sam = [(Y[f].astype(np.int64), up(U[f]).astype(np.int64), up(V[f]).astype(np.int64)) for f in win]
    c = sam[d]
    passes = [np.abs(c[0] - s[0]) + np.abs(c[1] - s[1]) + np.abs(c[2] - s[2]) <= thresh for s in sam]
    count = np.sum(passes, axis=0).astype(np.int64)
    assert count.min() >= 1
    out = []
    for k in range(3):
        if variant == "rational":
            total = sum(np.where(p, s[k], 0) for p, s in zip(passes, sam))
            out.append(((2 * total + count) // (2 * count)).astype(dt))
            continue
        factor = np.float32(1) / count.astype(np.float32)
        acc = np.full((h, w), 0.5, np.float32)
        order = range(len(win) - 1, -1, -1) if variant == "reversed" else range(len(win))
        for i in order:
            s = sam[i][k].astype(np.float32)
            if variant == "fma":
                step = (factor.astype(np.float64) * s.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
            else:
                prod = factor * s
                assert prod.dtype == np.float32
                step = acc + prod
            acc = np.where(passes[i], step, acc).astype(np.float32)
        out.append(acc.astype(np.int64).astype(dt))                  # (T) by truncation; the sums are positive and below the type's range
    # a chroma sample takes the value of ONE luma pixel: the even column of the first luma row that maps to its row
    ccy = np.arange(h // 2)
    ly = (2 * (ccy & ~1) + (ccy & 1)) if interlaced else 2 * ccy
    pick = lambda a: a[ly][:, 0::2]
    return out[0], pick(out[1]), pick(out[2]), count


def filter_clip(planes, d, threshold, bits, interlaced=False, variant="ref", frames=None):
    """(Y, U, V, count) of the output frames `frames` (default: all), stacked"""
    frames = range(planes[0].shape[0]) if frames is None else frames
    res = [filter_frame(planes, t, d, threshold, bits, interlaced, variant) for t in frames]
    return tuple(np.stack([r[k] for r in res]) for k in range(4))


def make_clip(n, w, h, bits, threshold, rng):
    """the generator of tests/test_gpu_temporal_nr.py: two scenes with a cut at n // 2 - 1, the second base far from the first; per-frame
    noise on 60 % of the samples, uniform in +-max(1, thresh) on Y and +-max(1, thresh // 3) on U and V"""
    thresh = threshold << (bits - 8)
    maxv = (1 << bits) - 1
    dt = np.uint8 if bits <= 8 else np.uint16
    cut = n // 2 - 1
    ay, ac = max(1, thresh), max(1, thresh // 3)
    planes = []
    for (hh, ww, amp) in ((h, w, ay), (h // 2, w // 2, ac), (h // 2, w // 2, ac)):
        lo, hi = amp, maxv - amp
        base1 = rng.integers(lo, max(lo + 1, maxv // 3), (hh, ww))
        base2 = rng.integers(min(hi, 2 * maxv // 3), hi + 1, (hh, ww))
        fr = []
        for f in range(n):
            base = base1 if f <= cut else base2
            noise = rng.integers(-amp, amp + 1, (hh, ww)) * (rng.random((hh, ww)) < 0.6)
            fr.append(np.clip(base + noise, 0, maxv))
        planes.append(np.stack(fr).astype(dt))
    return tuple(planes)
