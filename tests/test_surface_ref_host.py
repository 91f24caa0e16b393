"""The surface helper of the decoder-surface tests (tests/surface_clips.py), pinned on the CPU: to_surfaces / from_surfaces round-trip every
layout, the padding holds its poison, and the low bits under MSB-aligned samples really are non-zero -- a device path that forgot the shift,
or masked instead of shifting, cannot pass the GPU tests by accident."""
import numpy as np
import pytest

import surface_clips as SC

LAYOUTS = [(8, 1, 0), (8, 0, 0), (10, 1, 1), (10, 0, 1), (10, 1, 0), (12, 1, 1), (12, 0, 1), (12, 1, 0), (16, 1, 1)]


def lsb_clip(rng, n, W, H, bits):
    dt = np.uint8 if bits <= 8 else np.uint16
    return {"Y": rng.integers(0, 1 << bits, (n, H, W)).astype(dt), "U": rng.integers(0, 1 << bits, (n, H // 2, W // 2)).astype(dt),
            "V": rng.integers(0, 1 << bits, (n, H // 2, W // 2)).astype(dt)}


@pytest.mark.parametrize("bits,interleaved,msb", LAYOUTS)
def test_round_trip(bits, interleaved, msb):
    rng = np.random.default_rng(bits * 4 + interleaved * 2 + msb)
    W, H, n = 22, 12, 3
    clip = lsb_clip(rng, n, W, H, bits)
    fill = 0xA5 if bits == 8 else 0xA5A5
    s = SC.to_surfaces(clip, bits, interleaved, msb, rng, padY=5, padUV=3, fill=fill)
    dt = np.uint8 if bits == 8 else np.uint16
    assert s["Y"].dtype == dt and s["Y"].shape == (n, H, W + 5) and np.all(s["Y"][:, :, W:] == fill)
    if interleaved:
        assert s["V"] is None and s["U"].shape == (n, H // 2, W + 3) and np.all(s["U"][:, :, W:] == fill)
        # U0 V0 U1 V1 ...
        sh = 16 - bits if msb else 0
        assert np.array_equal(s["U"][:, :, 0:W:2] >> sh, clip["U"]) and np.array_equal(s["U"][:, :, 1:W:2] >> sh, clip["V"])
    else:
        assert s["U"].shape == s["V"].shape == (n, H // 2, W // 2 + 3) and np.all(s["V"][:, :, W // 2:] == fill)
    back = SC.from_surfaces(s, W, H, bits, interleaved, msb)
    for k in "YUV":
        assert back[k].dtype == clip[k].dtype and np.array_equal(back[k], clip[k]), k


@pytest.mark.parametrize("bits", [9, 10, 12, 15])
def test_low_bits_under_msb_samples_are_never_zero(bits):
    rng = np.random.default_rng(bits)
    clip = lsb_clip(rng, 2, 16, 8, bits)
    for interleaved in (0, 1):
        s = SC.to_surfaces(clip, bits, interleaved, 1, rng)
        mask = (1 << (16 - bits)) - 1
        for k in "YUV":
            if s[k] is not None:
                low = s[k] & mask
                assert low.min() >= 1, (k, "a zero low-bit field: the container equals sample << shift and hides a missing shift's error")
                if mask > 1:
                    assert len(np.unique(low)) > 1
        # ... so reading the containers as samples, or masking the low bits away without shifting, is wrong everywhere
        assert not np.any(s["Y"] == clip["Y"])
        assert np.array_equal(s["Y"] >> (16 - bits), clip["Y"])


def test_msb_at_8_bits_is_refused_by_the_helper():
    rng = np.random.default_rng(0)
    with pytest.raises(AssertionError):
        SC.to_surfaces(lsb_clip(rng, 1, 4, 4, 8), 8, 1, 1, rng)


def test_crop_uses_the_chroma_origin_of_the_abi():
    rng = np.random.default_rng(1)
    clip = lsb_clip(rng, 1, 32, 16, 8)
    c = SC.crop(clip, 6, 2, 10, 8)            # chroma origin 3, 1; 5 x 4 chroma samples
    assert c["Y"].shape == (1, 8, 10) and c["U"].shape == (1, 4, 5)
    assert np.array_equal(c["U"], clip["U"][:, 1:5, 3:8]) and np.array_equal(c["V"], clip["V"][:, 1:5, 3:8])
