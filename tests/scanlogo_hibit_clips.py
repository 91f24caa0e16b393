"""The clips of the high-bit ScanLogo tests (test_scanlogo_ref_host.py on the CPU, test_gpu_scanlogo_hibit.py on the device), each made
once per depth and never written to, with the CPU reference's .lgd (tests/scanlogo_ref.py) computed once per process."""
import numpy as np

import amt_synth as S

THY, QUOTA, SID = 12, 25, 1041        # (thy is in container units at every depth: the flat frames' rings are exactly flat)

# name -> (W, H, logo w, logo h, x, y, frames, seed, period, fade, flat_every)
CLIPS = {
    "A": (352, 240, 96, 48, 224, 18, 60, 0x5EED0004, 20, 4, 2),          # the clip of test_gpu_scanlogo_stream.py
    "odd": (352, 240, 66, 40, 226, 18, 60, 0x5EED0004, 20, 4, 2),        # chroma origin 113, wUV 33: the 2-byte lanes
    "grow": (64, 40, 48, 24, 8, 8, 300, 0x5EED0004, 20, 4, 1),           # every frame kept: the store outgrows its first 256 slots
    "auto": (640, 360, 128, 64, 480, 32, 240, 0x5EED00A1, 60, 6, 4),     # the clip of test_gpu_logofind.py
}
AUTO_RECT = (490, 34, 108, 56)        # what the finder's first candidate is on "auto" (8, 10 and 12 bits)

_clips, _refs = {}, {}


def geometry(name):
    W, H, lw, lh, x, y, n = CLIPS[name][:7]
    return W, H, lw, lh, x, y, n


def clip(name, bits):
    if (name, bits) not in _clips:
        W, H, lw, lh, x, y, n, seed, period, fade, flat = CLIPS[name]
        _, alpha, alphaUV = S.make_logo(lw, lh)
        c = S.make_clip_np(n, W, H, seed, alpha, alphaUV, x, y, bits=bits, period=period, fade=fade, flat_every=flat)
        for a in c.values():
            a.setflags(write=False)
        _clips[(name, bits)] = c
    return _clips[(name, bits)]


def clean(name, bits):
    """the same frames without the logo (alpha 0: the flat frames stay)"""
    W, H, lw, lh, x, y, n, seed, period, fade, flat = CLIPS[name]
    _, alpha, alphaUV = S.make_logo(lw, lh)
    return S.make_clip_np(n, W, H, seed, np.zeros_like(alpha), np.zeros_like(alphaUV), x, y, bits=bits, period=period, fade=fade,
                          flat_every=flat)


def presence(name):
    n, period, fade = CLIPS[name][6], CLIPS[name][8], CLIPS[name][9]
    return S.logo_presence(np.arange(n), period, fade)


def reference(orc, name, bits, tmpdir, rect=None, quota=QUOTA):
    """(.lgd bytes, info) of scanlogo_ref.scanlogo over the clip; rect: (x, y, w, h), default the logo's own rectangle"""
    import scanlogo_ref as R
    W, H, lw, lh, x, y, n = geometry(name)
    rect = rect or (x, y, lw, lh)
    key = (name, bits, rect, quota)
    if key not in _refs:
        path = tmpdir / ("ref_%s_%d_%d_%d.lgd" % (name, bits, rect[0], min(quota, 999999)))
        _refs[key] = R.scanlogo(orc, clip(name, bits), bits, W, H, *rect, THY, quota, path=path, serviceid=SID)
    return _refs[key]
