"""Numpy restatement of the deband on decoder surfaces (amtgpu_deband_run_surfaces, include/amt_gpu.h; DESIGN.md section 6f, "surfaces in
kind"), written from the rule by composing what exists and not from the kernels, the way tests/resize_surfaces_ref.py is: de-interleave
U and V, shift the containers to samples, apply the planar restatement (deband_ref.filter_clip, which tests/test_deband_host.py holds
against the rule's text and the C++ tables), shift back and re-interleave.  No row is copied: every output container has zero low bits.
Checker side only."""
import numpy as np

import deband_ref as R
import temporal_nr_surfaces_ref as TS


def deband_surfaces(planes, bits, interleaved, msb, radius=25, threshold=1, sample=2, blur_first=True, seed=0, offsets=None):
    """the destination's tight planes -- (Y, UV) interleaved, (Y, U, V) planar -- over the source's tight planes (containers as stored).
    offsets: the three COMPONENT planes' (dx, dy), as deband_ref.filter_clip takes them"""
    out = R.filter_clip(TS.unpack(planes, bits, interleaved, msb), bits, radius, threshold, sample, blur_first, seed, offsets)
    return TS.pack(out, bits, interleaved, msb)


def interleaved_table(u, v):
    """one of dx / dy of the UV plane walked as one plane: U's entry at 2x, V's at 2x + 1"""
    return np.stack([u, v], -1).reshape(u.shape[0], 2 * u.shape[1])
