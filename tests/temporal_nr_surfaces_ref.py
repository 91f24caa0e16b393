"""Numpy restatement of the temporal noise reduction on decoder surfaces (amtgpu_temporal_nr_surfaces, include/amt_gpu.h; DESIGN.md
section 9, "surfaces in kind"), written from the rule by composing what exists and not from the kernel: de-interleave U and V, shift the
containers to samples, apply the planar restatement (temporal_nr_ref.filter_clip, which tests/test_temporal_nr_host.py holds against the
compiled reference), shift back and re-interleave.  Nothing is copied from the source: every output container has zero low bits.
Checker side only."""
import numpy as np

import temporal_nr_ref as R

# kind: (interleaved, msb) of the layouts the entry point takes; "planar" is the planar LSB pair that runs the planar kernel
KINDS = {"nv12": (True, False), "interleaved-lsb": (True, False), "p0xx": (True, True), "planar-msb": (False, True), "planar": (False, False)}


def shift_of(bits, msb):
    return 16 - bits if msb else 0


def kinds_of(bits):
    """the kinds a clip of this depth can be stored in"""
    return ["nv12", "planar"] if bits == 8 else ["interleaved-lsb", "p0xx", "planar-msb", "planar"]


def split_planes(planes, interleaved):
    """(Y, U, V) container planes of a surface's tight planes: (Y, UV [n, h/2, w]) when interleaved, U the even and V the odd containers"""
    if not interleaved:
        return tuple(planes)
    Y, UV = planes
    return Y, UV[:, :, 0::2], UV[:, :, 1::2]


def join_planes(yuv, interleaved):
    if not interleaved:
        return tuple(yuv)
    Y, U, V = yuv
    UV = np.empty(U.shape[:2] + (2 * U.shape[2],), U.dtype)
    UV[:, :, 0::2], UV[:, :, 1::2] = U, V
    return Y, UV


def pack(samples, bits, interleaved, msb, rng=None):
    """the surface's tight planes that hold these (Y, U, V) samples: container = sample << s, with random NON-ZERO low bits from rng
    where there are any (s > 0)"""
    s = shift_of(bits, msb)
    out = []
    for p in samples:
        c = (p.astype(np.uint32) << s).astype(p.dtype)
        if s and rng is not None:
            c |= rng.integers(1, 1 << s, p.shape).astype(p.dtype)
        out.append(c)
    return join_planes(out, interleaved)


def unpack(planes, bits, interleaved, msb):
    """(Y, U, V) samples of a surface's tight planes"""
    s = shift_of(bits, msb)
    return tuple(np.ascontiguousarray(p >> s) for p in split_planes(planes, interleaved))


def filter_surfaces(planes, d, threshold, bits, interleaved, msb, il_chroma=False, frames=None):
    """(the destination's tight planes -- (Y, UV) interleaved, (Y, U, V) planar --, count [n, h, w]) of the output frames `frames`
    (default: all) over the source's tight planes (containers as stored).  il_chroma: the interlaced 4:2:0 chroma rows"""
    s = shift_of(bits, msb)
    Y, U, V, count = R.filter_clip(unpack(planes, bits, interleaved, msb), d, threshold, bits, il_chroma, frames=frames)
    dt = planes[0].dtype
    out = [(p.astype(np.uint32) << s).astype(dt) for p in (Y, U, V)]
    return join_planes(out, interleaved), count
