"""Decoder surfaces (AmtGpuSurfaces: NV12, P010 / P012, planar MSB) made from planar LSB numpy clips, and back, for the tests: the numpy
statement of the layouts amtgpu_surfaces_extract_rect, amtgpu_scanlogo_stream_feed_surfaces, amtgpu_logofind_add_surfaces and
amtgpu_weave_fields_batch_msb read."""
import numpy as np


def msb_containers(a, bits, rng):
    """the samples of a (uint16, below 1 << bits) in the high bits of their containers, with random NON-ZERO low bits under every one
    (what a dithering filter or a sloppy decoder leaves there; nothing below 16 bits to fill at bits == 16)"""
    shift = 16 - bits
    a = np.asarray(a).astype(np.uint16)
    if shift == 0:
        return a.copy()
    low = rng.integers(1, 1 << shift, a.shape, dtype=np.uint16)
    return ((a << shift) | low).astype(np.uint16)


def to_surfaces(clip, bits, interleaved, msb, rng, padY=0, padUV=0, fill=0xA5):
    """clip: {"Y": (N, H, W), "U" / "V": (N, H/2, W/2)} planar LSB samples (uint8 at 8 bits, uint16 above) -> {"Y", "U", "V"} surfaces:
    rows padY / padUV containers longer, the padding holding `fill`; interleaved: "U" is the U0 V0 U1 V1 ... plane (W + padUV containers a
    row) and "V" is None; msb: every container is sample << (16 - bits) with random non-zero low bits (msb_containers)"""
    assert not (msb and bits == 8), "MSB alignment needs 16-bit containers"
    dt = np.uint8 if bits <= 8 else np.uint16

    def cont(a):
        return msb_containers(a, bits, rng) if msb else np.asarray(a).astype(dt)

    def pad(a, n):
        out = np.full(a.shape[:2] + (a.shape[2] + n,), fill, dt)
        out[:, :, :a.shape[2]] = a
        return out

    Y, U, V = cont(clip["Y"]), cont(clip["U"]), cont(clip["V"])
    if interleaved:
        UV = np.empty(U.shape[:2] + (2 * U.shape[2],), dt)
        UV[:, :, 0::2] = U
        UV[:, :, 1::2] = V
        return {"Y": pad(Y, padY), "U": pad(UV, padUV), "V": None}
    return {"Y": pad(Y, padY), "U": pad(U, padUV), "V": pad(V, padUV)}


def from_surfaces(surf, W, H, bits, interleaved, msb):
    """the inverse: the planar LSB clip the surfaces describe (sample = container >> (16 - bits) when msb)"""
    shift = 16 - bits if msb else 0
    wUV = W // 2

    def samples(a):
        return (a >> shift).astype(a.dtype) if shift else a.copy()

    Y = samples(surf["Y"][:, :H, :W])
    if interleaved:
        U, V = samples(surf["U"][:, :H // 2, 0:2 * wUV:2]), samples(surf["U"][:, :H // 2, 1:2 * wUV:2])
    else:
        U, V = samples(surf["U"][:, :H // 2, :wUV]), samples(surf["V"][:, :H // 2, :wUV])
    return {"Y": Y, "U": U, "V": V}


def crop(clip, x, y, w, h):
    """the rectangle of a planar clip: chroma origin x >> 1, y >> 1, size w/2 x h/2"""
    cx, cy = x >> 1, y >> 1
    return {"Y": clip["Y"][:, y:y + h, x:x + w], "U": clip["U"][:, cy:cy + h // 2, cx:cx + w // 2],
            "V": clip["V"][:, cy:cy + h // 2, cx:cx + w // 2]}
