"""The resize rule of DESIGN.md section 6e restated in numpy and plain Python floats, from its text and not from the C++ plan
(amatsukaze_amd/csrc/resize_plan.cpp): the program of one axis, the two stages on a plane, a clip of three planes, and the float64
evaluation of the continuous definition on the same windows, with no quantisation anywhere, that the host test bounds the integers with.

Transcendentals come from `math` (the platform's libm, which the C++ plan calls too) and every double operation is written in the order
of the rule's text, so that the tables can be compared entry for entry."""
import functools
import math

import numpy as np

ONE, SHIFT, HALF = 16384, 14, 8192
KERNELS = {"blackman": 0, "lanczos": 1, "bilinear": 2}
DEFAULT_TAPS = {"blackman": 4, "lanczos": 3, "bilinear": 1}


def kernel_value(kernel, taps, x):
    ax = abs(x)
    if ax >= taps:
        return 0.0
    if ax == 0.0:
        return 1.0
    if kernel == "bilinear":
        return max(0.0, 1.0 - ax)
    px = math.pi * ax
    if kernel == "blackman":
        return math.sin(px) / px * (0.42 + 0.5 * math.cos(px / taps) + 0.08 * math.cos(2 * px / taps))
    if kernel == "lanczos":
        return math.sin(px) / px * math.sin(px / taps) / (px / taps)
    raise ValueError(kernel)


@functools.lru_cache(maxsize=None)
def _program(S, D, kernel, taps):
    scale = D / S
    fstep = min(scale, 1.0)
    support = taps / fstep
    K0 = math.ceil(2 * support)
    K = min(K0, S)
    start = np.zeros(D, np.int64)
    C = np.zeros((D, K), np.int64)
    W = np.zeros((D, K), np.float64)                                # the normalised weights, unquantised, in the same windows
    for i in range(D):
        c = (i + 0.5) / scale - 0.5
        lo = math.floor(c - support) + 1
        folded, total = {}, 0.0
        for p in range(lo, lo + K0):
            w = kernel_value(kernel, taps, (p - c) * fstep)
            total += w
            q = min(max(p, 0), S - 1)
            folded[q] = folded.get(q, 0.0) + w
        pos = sorted(folded)
        q = [math.floor(folded[p] / total * ONE + 0.5) for p in pos]
        best = max(range(len(q)), key=lambda j: (q[j], -j))         # the largest, the lowest position among equals
        q[best] += ONE - sum(q)
        st = min(max(lo, 0), S - K)
        start[i] = st
        for p, v in zip(pos, q):
            if v:
                assert 0 <= p - st < K, (S, D, i, p, st, K)
                C[i, p - st] = v
            if 0 <= p - st < K:
                W[i, p - st] = folded[p] / total
    for a in (start, C, W):
        a.setflags(write=False)
    return K, start, C, W


def program(S, D, kernel="blackman", taps=None):
    """(K, start[D], C[D][K]) of one axis"""
    taps = DEFAULT_TAPS[kernel] if not taps or taps <= 0 or kernel == "bilinear" else taps
    return _program(S, D, kernel, taps)[:3]


def float_program(S, D, kernel="blackman", taps=None):
    """(K, start[D], W[D][K]): the continuous definition's normalised weights in the integer program's windows"""
    taps = DEFAULT_TAPS[kernel] if not taps or taps <= 0 or kernel == "bilinear" else taps
    K, start, _, W = _program(S, D, kernel, taps)
    return K, start, W


REGION_BYTES, REGION_SLACK = 2048, 48


def windows(S, D, kernel="blackman", taps=None):
    """(K, start[D]) of one axis without its coefficients: the windows alone, which is all the horizontal stage's staging depends on
    (tests/test_resize_host.py holds them against program()'s)"""
    taps = DEFAULT_TAPS[kernel] if not taps or taps <= 0 or kernel == "bilinear" else taps
    scale = D / S
    support = taps / min(scale, 1.0)
    K = min(math.ceil(2 * support), S)
    start = [min(max(math.floor((i + 0.5) / scale - 0.5 - support) + 1, 0), S - K) for i in range(D)]
    return K, np.array(start, np.int64)


def columns_per_wave(S, D, es, kernel="blackman", taps=None):
    """(cpw, K, spans): the run of output columns a wave of the horizontal stage takes, from the rule's text: a
    wave stages the source span of its run, start[last] + K - start[first] samples of es bytes, in a region of 2048 bytes of which 48
    are kept for the aligned-down front and the zero taps behind; the run is halved from 64 until every run of the row fits.  spans:
    each run's span in bytes, in the row's order.  cpw 0, spans (): not even single columns fit, which the create refuses"""
    K, start = windows(S, D, kernel, taps)
    cpw = 64
    while cpw >= 1:
        spans = tuple(int(start[min(c0 + cpw, D) - 1] + K - start[c0]) * es for c0 in range(0, D, cpw))
        if all(s + REGION_SLACK <= REGION_BYTES for s in spans):
            return cpw, K, spans
        cpw //= 2
    return 0, K, ()


def stage(lines, prog, maxv):
    """the sample rule along the LAST axis of `lines` (any leading shape): int64 in, int64 out"""
    K, start, C = prog
    idx = start[:, None] + np.arange(K)[None, :]
    out = np.empty(lines.shape[:-1] + (len(start),), np.int64)
    flat_in, flat_out = lines.reshape(-1, lines.shape[-1]), out.reshape(-1, len(start))
    for r in range(0, flat_in.shape[0], 64):
        acc = (flat_in[r:r + 64][:, idx].astype(np.int64) * C[None]).sum(axis=-1)
        assert acc.max(initial=0) + HALF < 2 ** 31 and acc.min(initial=0) + HALF >= -2 ** 31
        flat_out[r:r + 64] = np.clip((acc + HALF) >> SHIFT, 0, maxv)
    return out


def resize_plane(plane, dst_w, dst_h, bits, kernel="blackman", taps=None):
    """plane (..., S_h, S_w) of containers -> (..., dst_h, dst_w), horizontal stage first"""
    maxv = (1 << bits) - 1
    S_h, S_w = plane.shape[-2:]
    mid = stage(plane.astype(np.int64), program(S_w, dst_w, kernel, taps), maxv)                   # (..., S_h, D_w)
    out = stage(np.swapaxes(mid, -1, -2), program(S_h, dst_h, kernel, taps), maxv)                 # (..., D_w, D_h)
    return np.ascontiguousarray(np.swapaxes(out, -1, -2)).astype(plane.dtype)


def resize_clip(planes, dst_w, dst_h, bits, kernel="blackman", taps=None):
    """(Y, U, V) of (N, h, w), (N, h/2, w/2) x 2 -> the three resized planes; every plane on its own, chroma S/2 -> D/2"""
    Y, U, V = planes
    assert dst_w % 2 == 0 and dst_h % 2 == 0 and Y.shape[-1] % 2 == 0 and Y.shape[-2] % 2 == 0
    return (resize_plane(Y, dst_w, dst_h, bits, kernel, taps), resize_plane(U, dst_w // 2, dst_h // 2, bits, kernel, taps),
            resize_plane(V, dst_w // 2, dst_h // 2, bits, kernel, taps))


def float_stage(lines, fprog):
    K, start, W = fprog
    idx = start[:, None] + np.arange(K)[None, :]
    return (lines[..., idx] * W).sum(axis=-1)


def resize_plane_float(plane, dst_w, dst_h, bits, kernel="blackman", taps=None):
    """the same two stages in float64 with unquantised weights and no rounding; each stage's result is clamped to 0 .. maxv as the
    sample rule clamps (a clamp moves two values no further apart, so a bound on the difference before it holds behind it)"""
    maxv = float((1 << bits) - 1)
    mid = np.clip(float_stage(plane.astype(np.float64), float_program(plane.shape[-1], dst_w, kernel, taps)), 0.0, maxv)
    out = np.clip(float_stage(np.swapaxes(mid, -1, -2), float_program(plane.shape[-2], dst_h, kernel, taps)), 0.0, maxv)
    return np.swapaxes(out, -1, -2)


def make_clip(n, w, h, bits, rng):
    """seeded noise over the whole range of the depth"""
    dt = np.uint8 if bits <= 8 else np.uint16
    mk = lambda hh, ww: rng.integers(0, 1 << bits, (n, hh, ww)).astype(dt)
    return mk(h, w), mk(h // 2, w // 2), mk(h // 2, w // 2)
