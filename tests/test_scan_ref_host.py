"""tests/scan_ref.py (the numpy statement of LogoScan::AddFrame the GPU shape tests compare with) against the C++ oracle at 8 bits:
the accept / reject decision of every frame and all five sums of every pixel.  CPU only."""
import numpy as np
import pytest

import scan_ref
from amtlib import Oracle, _ptr
from scan_clips import make_scan_clip

RECTS = [(2, 2), (4, 2), (6, 4), (98, 50), (262, 34), (520, 18), (34, 130)]


@pytest.mark.parametrize("thy", [0, 3, 12])
@pytest.mark.parametrize("w,h", RECTS)
def test_scan_ref_matches_oracle_u8(w, h, thy):
    rng = np.random.RandomState(0x5CA0 + 131 * w + 7 * h + thy)
    W, H, x0, y0 = w + 22, h + 14, 6, 4
    n = 40
    plan = []
    for i in range(n):
        if i % 5 == 4:                                   # every fifth frame: one plane's spread is thy + 1
            s = [int(rng.randint(0, thy + 1)) for _ in range(3)]
            s[(0, 2, 1)[(i // 5) % 3] if min(w, h) > 2 else 0] = thy + 1      # (a 2x2 rectangle's chroma ring is a single sample)
            plan.append(dict(spread=tuple(s)))
        elif i % 5 == 0:
            plan.append(dict(spread=(thy, thy, thy)))    # exactly on the edge: accepted
        else:
            plan.append(dict(spread=tuple(int(rng.randint(0, thy + 1)) for _ in range(3))))
    clip, info = make_scan_clip(rng, W, H, 10, 8, (x0, y0, w, h), plan)
    Y, U, V = clip["Y"], clip["U"], clip["V"]
    orc = Oracle()
    so = orc.lib.orc_scan_create(w, h, 1, 1, thy)
    acc = scan_ref.ScanAccumulator(w, h, thy)
    want, got = [], []
    for i in range(n):
        y, u, v = Y[i, y0:, x0:], U[i, y0 // 2:, x0 // 2:], V[i, y0 // 2:, x0 // 2:]
        want.append(orc.lib.orc_scan_add_frame_u8(so, y.ctypes.data, u.ctypes.data, v.ctypes.data, Y.shape[2], U.shape[2]))
        got.append(int(acc.add(y, u, v)))
    assert got == want
    assert want == [int(all(sp <= thy for _, sp in rec)) for rec in info]          # the generator's spreads are the real ones
    assert 0 < sum(want) < n and acc.nframes == sum(want) == orc.lib.orc_scan_nframes(so)
    osum = np.zeros(acc.npx * 5)
    orc.lib.orc_scan_sums(so, _ptr(osum))
    orc.lib.orc_scan_free(so)
    osum = osum.reshape(acc.npx, 5)                      # F, B, F2, B2, FB
    s, p = acc.sums()
    s = s.reshape(acc.npx, 3)
    assert np.array_equal(s[:, 0], osum[:, 0].astype(np.int64))
    assert np.array_equal(s[:, 1], osum[:, 2].astype(np.int64))
    assert np.array_equal(s[:, 2], osum[:, 4].astype(np.int64))
    ysz, csz = w * h, (w // 2) * (h // 2)
    for k, o in enumerate((0, ysz, ysz + csz)):
        assert np.all(osum[o:o + (ysz if k == 0 else csz), 1] == p[2 * k]) and np.all(osum[o:o + (ysz if k == 0 else csz), 3] == p[2 * k + 1])


def test_med_average_rounds_half_up_in_double():
    """(t + nn/2) / nn truncated: nn = 4 -> adds 2, so a trimmed sum of 4k+2 rounds up and 4k+1 rounds down; nn odd adds nn//2"""
    s = np.array([0, 0, 10, 10, 11, 11, 90, 90])         # middle half 10 10 11 11 -> (42 + 2) / 4 = 11
    assert scan_ref.med_average(s) == 11
    s = np.array([0, 0, 10, 10, 10, 11, 90, 90])         # 41 + 2 -> 10
    assert scan_ref.med_average(s) == 10
    assert scan_ref.med_average(np.array([7, 8])) == 8   # (15 + 1) / 2
    assert scan_ref.med_average(np.array([5, 5])) == 5


def test_one_row_plane_is_pushed_twice():
    p = np.array([[3, 9, 4]])
    assert scan_ref.border_samples(p, 3, 1).tolist() == [3, 3, 4, 4, 9, 9]
    p = np.arange(20).reshape(4, 5)
    assert scan_ref.border_samples(p, 5, 4).tolist() == sorted([0, 1, 2, 3, 4, 15, 16, 17, 18, 19, 5, 9, 10, 14])
