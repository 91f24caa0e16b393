"""Inputs of the frame metrics on decoder surfaces (tests/test_gpu_surface_stats.py), shared with tests/test_surface_stats_abi.py, which
shows without a GPU that every one of them tells the right records from those of two wrong kernels.

A case is an allocation of N + 1 MSB-aligned Y surfaces (plane_edge_clips.embed: row padding, two rows after each surface -- the gap
between surfaces -- and the rows after the last all hold 0xFFFF): surface 0 is the picture before the batch, surfaces 1..N the batch.
The truth is oracle/frame_stats_oracle.py's frame_metrics on container >> shift.
"""
from __future__ import annotations

import numpy as np

import plane_edge_clips as P
import surface_clips as SC
from plane_edge_clips import FS

# (W, pitch) per 16-bit form of frame_stats_kernel
FORMS = {"buf": (64, 64), "buf_ragged": (37, 48), "plain": (37, 37)}
DEPTHS = (9, 10, 12, 15)                      # shifts 7, 6, 4, 1
BATCHES = (1, 2, 33, 65)                      # odd; even; across the 32-frame run (its first frame's predecessor is re-read, shifted); an odd last run


def heights(form):
    """the minimum; one exact 16-row tile; a partial last tile; more than one tile with halo rows; plain: a partial last tile of its 8 rows"""
    return (4, 16, 21, 33) + ((9,) if form == "plain" else ())


# (form, bits, H, N, kind)   kind: 'random' (random samples, random non-zero low bits) or 'alternating' (0 / maxv along a row, every low bit set)
GEOMETRY_CASES = [(f, b, H, 2, "random") for f in FORMS for b in DEPTHS for H in heights(f)]
BATCH_CASES = [(f, DEPTHS[(i + j) % 4], 21, N, "random") for i, f in enumerate(FORMS) for j, N in enumerate(BATCHES)]
LOW_BITS_CASES = [(f, b, 21, 3, "alternating") for f in FORMS for b in DEPTHS]
CASES = GEOMETRY_CASES + BATCH_CASES + LOW_BITS_CASES


def case_id(case):
    f, bits, H, N, kind = case
    return f"{f}-{bits}b-h{H}-n{N}-{kind}"


def containers(case, extra_seed=0):
    """(N + 1, H, W) uint16 MSB-aligned containers of the case"""
    f, bits, H, N, kind = case
    W, pitch = FORMS[f]
    shift = 16 - bits
    rng = np.random.default_rng([bits, W, pitch, H, N, extra_seed])
    if kind == "random":
        return SC.msb_containers(rng.integers(0, 1 << bits, (N + 1, H, W)), bits, rng)
    maxv = (1 << bits) - 1
    n, y, x = np.ogrid[:N + 1, :H, :W]
    s = (((x + y // 2 + n) & 1) * maxv).astype(np.uint16)
    return ((s << shift) | ((1 << shift) - 1)).astype(np.uint16)


def clip_of(case):
    """(allocation of N + 1 surfaces, one separate surface for the `prev in another allocation` run)"""
    f, bits, H, N, kind = case
    W, pitch = FORMS[f]
    clip = P.embed(containers(case), pitch, rows_after=2)
    sep = P.embed(containers((f, bits, H, 0, "random"), extra_seed=1), pitch, base=3)
    assert clip.form() == f and sep.form() == f
    return clip, sep


def runs_of(case):
    """the (batch, previous picture or None) pairs the GPU test runs"""
    clip, sep = clip_of(case)
    return [(clip.sub(1), None), (clip.sub(1), clip.sub(0, 1)), (clip.sub(1), sep)]


def truth(batch, prev, bits):
    shift = 16 - bits
    return FS.frame_metrics(batch.frames() >> shift, None if prev is None else prev.frames()[0] >> shift)


# ---- two wrong kernels, as sample planes the oracle can take ----
def shift32_samples(frames, shift):
    """a 32-bit shift of the packed dwords without per-half handling: the discarded bits of the sample in a dword's high half (odd
    column) land in the top of its low neighbour (even column)"""
    c = frames.astype(np.int64)
    out = c >> shift
    hi = c[..., 1::2]
    out[..., 0:2 * hi.shape[-1]:2] |= (hi & ((1 << shift) - 1)) << (16 - shift)
    return out


def wrong_shift32(batch, prev, bits):
    shift = 16 - bits
    return FS.frame_metrics(shift32_samples(batch.frames(), shift), None if prev is None else shift32_samples(prev.frames(), shift)[0])


def wrong_shifted_sums(batch, prev, bits):
    """the plain kernel on the containers as they are, its sums shifted afterwards"""
    return FS.frame_metrics(batch.frames(), None if prev is None else prev.frames()[0]) >> np.uint64(16 - bits)
