"""The reference of the surface erase tests (tests/surface_erase_ref.py), pinned on the CPU: for the planar LSB layout it is the oracle's
Delogo itself, for every layout the samples of rewritten frames are the oracle's, rewritten MSB containers have zero low bits, and every
container that is not rewritten -- outside the rectangle, an odd last chroma row in field mode, a {0, 0} frame -- still carries the
random non-zero low bits it had.  Each case holds a rewritten frame, an untouched {0, 0} frame and a field-mode frame over an odd hUV,
asserted, so that no comparison goes vacuous."""
import numpy as np
import pytest

import amt_synth as S
import surface_clips as SC
import surface_erase_ref as ER
from amtlib import Oracle

LAYOUTS = [(8, 1, 0), (10, 1, 1), (12, 1, 1), (16, 1, 1), (10, 0, 1), (10, 1, 0), (10, 0, 0)]     # (bits, interleaved, msb)
W, H, RECT = 64, 48, (20, 10, 26, 18)                                                              # hUV = 9: odd
FADES = np.array([(0.0, 0.0), (1.0, 1.0), (0.3, 0.8), (0.0, 0.0), (0.5, 0.5), (1.0, 0.0)], np.float32)


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def make(orc, bits, interleaved, msb):
    rng = np.random.default_rng(bits * 4 + interleaved * 2 + msb)
    n = len(FADES)
    dt = np.uint8 if bits <= 8 else np.uint16
    clip = {"Y": rng.integers(0, 1 << bits, (n, H, W)).astype(dt), "U": rng.integers(0, 1 << bits, (n, H // 2, W // 2)).astype(dt),
            "V": rng.integers(0, 1 << bits, (n, H // 2, W // 2)).astype(dt)}
    fill = 0xA5 if bits == 8 else 0xA5A5
    surf = SC.to_surfaces(clip, bits, interleaved, msb, rng, padY=6, padUV=4, fill=fill)
    x, y, lw, lh = RECT
    data = S.make_logo(lw, lh)[0]
    lo = orc.make_logo(data, lw, lh, W, H, x, y)
    return clip, surf, lo


@pytest.mark.parametrize("fade0_identity", [1, 0])
@pytest.mark.parametrize("bits,interleaved,msb", LAYOUTS)
def test_expected_surfaces(orc, bits, interleaved, msb, fade0_identity):
    clip, surf, lo = make(orc, bits, interleaved, msb)
    before = {k: (None if v is None else v.copy()) for k, v in surf.items()}
    exp = ER.expected_surfaces(orc, lo, surf, W, H, bits, interleaved, msb, RECT, FADES, fade0_identity)
    for k in "YUV":                                                            # the input is not modified
        assert (surf[k] is None and before[k] is None) or np.array_equal(surf[k], before[k])
    want = ER.oracle_planes(orc, lo, clip, bits, FADES)
    live = ER.rewritten_frames(FADES, bits, msb, fade0_identity)
    skipping = ER.skips_fade0(bits, msb, fade0_identity)
    assert skipping == bool(fade0_identity and (bits in (8, 16) or msb))
    # the case holds what it is meant to hold
    hUV = RECT[3] // 2
    assert hUV % 2 == 1 and any(f[0] != f[1] for f in FADES) and live[1] and (FADES[0] == 0).all()
    assert (not live[0] and not live[3]) if skipping else live.all()
    assert not np.array_equal(want["Y"][1], clip["Y"][1]) and not np.array_equal(want["U"][2], clip["U"][2])
    # planar LSB: the oracle's planes themselves (padding aside)
    if not interleaved and not msb:
        for k in "YUV":
            ww = W if k == "Y" else W // 2
            for f in np.nonzero(live)[0]:
                assert np.array_equal(exp[k][f][:, :ww], want[k][f]), k
            assert np.array_equal(exp[k][:, :, ww:], surf[k][:, :, ww:])
    # every layout: the samples of rewritten frames are the oracle's, the others' are the input's
    back = SC.from_surfaces(exp, W, H, bits, interleaved, msb)
    for k in "YUV":
        for f in range(len(FADES)):
            assert np.array_equal(back[k][f], want[k][f] if live[f] else clip[k][f]), (k, f)
    # rewritten containers: zero low bits; all others: bit for bit the input, which carries non-zero low bits under MSB samples
    mask = ER.rewritten_mask(surf, RECT, interleaved, FADES, live)
    low = (1 << (16 - bits)) - 1 if msb else 0
    for k in "YUV":
        if surf[k] is None:
            assert exp[k] is None
            continue
        m = mask[k]
        assert m.any() and not m.all()
        assert np.array_equal(exp[k][~m], surf[k][~m]), k
        if low:
            assert np.all(exp[k][m] & low == 0), k
            pic = np.zeros(m.shape, bool)
            pic[:, :, :(W if (k == "Y" or interleaved) else W // 2)] = True
            assert np.all(exp[k][~m & pic] & low != 0), k
    # field mode over an odd hUV: the last chroma row of the rectangle is the input's, the row above is rewritten
    x, y, lw, lh = RECT
    cy, cx = y // 2, x // 2
    f = 2
    assert FADES[f][0] != FADES[f][1] and live[f]
    assert np.array_equal(exp["U"][f, cy + hUV - 1], surf["U"][f, cy + hUV - 1])
    # ... while the row above it is rewritten, and in frame mode so is the last row (seen in the zeroed low bits of MSB containers; in
    # the samples wherever the oracle changed them, which the comparison with its planes above covers)
    if low:
        c0, c1 = (2 * cx, 2 * (cx + lw // 2)) if interleaved else (cx, cx + lw // 2)
        assert np.all(exp["U"][f, cy + hUV - 2, c0:c1] & low == 0) and np.all(exp["U"][f, cy + hUV - 1, c0:c1] & low != 0)
        assert np.all(exp["U"][1, cy + hUV - 1, c0:c1] & low == 0)
