"""What AMTEraseLogo.erase_surfaces must leave in a batch of decoder surfaces, stated with the CPU oracle and numpy: the oracle's Delogo on
the planar LSB clip the surfaces describe, written back as containers into exactly the containers the erase rewrites -- every other
container stays as it was, low bits included.  Pinned on the CPU by test_surface_erase_ref_host.py."""
import numpy as np

import surface_clips as SC
from amtlib import _ptr


def skips_fade0(bits, msb, fade0_identity):
    """frames with fades {0, 0} are left untouched when fade 0 is the identity for this logo and no container can hold a sample above maxv:
    8- and 16-bit containers, and MSB-aligned ones at any depth (LSB 9..15-bit containers are computed: Delogo's min clamps them)"""
    return bool(fade0_identity) and (bits == 8 or bits == 16 or bool(msb))


def rewritten_frames(fades, bits, msb, fade0_identity):
    """bool per frame: the erase rewrites its rectangle"""
    fades = np.asarray(fades, np.float32).reshape(-1, 2)
    zero = (fades[:, 0] == 0) & (fades[:, 1] == 0)
    return ~zero if skips_fade0(bits, msb, fade0_identity) else np.ones(len(fades), bool)


def chroma_rows(fade, hUV):
    """chroma rows of the rectangle a frame's erase rewrites: all in frame mode, 2 * (hUV / 2) in field mode (an odd last row stays)"""
    return hUV if fade[0] == fade[1] else 2 * (hUV // 2)


def oracle_planes(orc, lo, clip, bits, fades):
    """the oracle's Delogo, frame by frame, on a copy of the tight planar LSB clip"""
    want = {k: np.ascontiguousarray(clip[k]).copy() for k in "YUV"}
    for i in range(want["Y"].shape[0]):
        orc.lib.orc_erase_frame(lo, _ptr(want["Y"][i]), _ptr(want["U"][i]), _ptr(want["V"][i]), want["Y"].shape[2], want["U"].shape[2], bits,
                                float(fades[i][0]), float(fades[i][1]))
    return want


def expected_surfaces(orc, lo, surf, W, H, bits, interleaved, msb, rect, fades, fade0_identity):
    """surf: {"Y", "U", "V"} surfaces of W x H pictures (surface_clips.to_surfaces; rows may be longer than the picture); rect = (x, y, w, h)
    of the logo `lo` (an oracle logo made for W x H at (x, y)); fades [n, 2].  Returns the surfaces after the erase: oracle_sample << shift
    in every rewritten container, every other container as it was."""
    fades = np.asarray(fades, np.float32).reshape(-1, 2)
    shift = 16 - bits if msb else 0
    x0, y0, lw, lh = rect
    cx, cy, wUV, hUV = x0 >> 1, y0 >> 1, lw >> 1, lh >> 1
    clip = SC.from_surfaces(surf, W, H, bits, interleaved, msb)
    want = oracle_planes(orc, lo, clip, bits, fades)
    out = {k: (None if v is None else v.copy()) for k, v in surf.items()}
    dt = out["Y"].dtype

    def cont(a):
        return (a.astype(np.uint32) << shift).astype(dt)

    live = rewritten_frames(fades, bits, msb, fade0_identity)
    for f in range(len(fades)):
        if not live[f]:
            continue
        out["Y"][f, y0:y0 + lh, x0:x0 + lw] = cont(want["Y"][f, y0:y0 + lh, x0:x0 + lw])
        rows = chroma_rows(fades[f], hUV)
        u = cont(want["U"][f, cy:cy + rows, cx:cx + wUV])
        v = cont(want["V"][f, cy:cy + rows, cx:cx + wUV])
        if interleaved:
            out["U"][f, cy:cy + rows, 2 * cx:2 * (cx + wUV):2] = u
            out["U"][f, cy:cy + rows, 2 * cx + 1:2 * (cx + wUV):2] = v
        else:
            out["U"][f, cy:cy + rows, cx:cx + wUV] = u
            out["V"][f, cy:cy + rows, cx:cx + wUV] = v
    return out


def rewritten_mask(surf, rect, interleaved, fades, live):
    """bool arrays shaped like the surfaces: True on every container the erase rewrites"""
    x0, y0, lw, lh = rect
    cx, cy, wUV, hUV = x0 >> 1, y0 >> 1, lw >> 1, lh >> 1
    m = {k: (None if v is None else np.zeros(v.shape, bool)) for k, v in surf.items()}
    for f in range(len(fades)):
        if not live[f]:
            continue
        m["Y"][f, y0:y0 + lh, x0:x0 + lw] = True
        rows = chroma_rows(fades[f], hUV)
        if interleaved:
            m["U"][f, cy:cy + rows, 2 * cx:2 * (cx + wUV)] = True
        else:
            m["U"][f, cy:cy + rows, cx:cx + wUV] = True
            m["V"][f, cy:cy + rows, cx:cx + wUV] = True
    return m
