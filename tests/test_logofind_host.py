"""Automatic logo detection, host half (amtgpu_logofind_candidates_host): sums stated in numpy (tests/logofind_ref.py) from small
synthetic clips -> ranked candidate rectangles.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import logofind_ref as LF


@pytest.fixture(scope="module")
def lib():
    from amatsukaze_amd import build as b
    b.build()
    from amatsukaze_amd import binding
    return binding.load()


def noise_clip(N, W, H, seed=1, lo=60, amp=40):
    """moving noise: every sample of every frame its own value in [lo, lo + amp)"""
    return np.random.RandomState(seed).randint(lo, lo + amp, size=(N, H, W)).astype(np.int64)


def put_square(Y, x0, y0, w, h, v):
    Y[:, y0:y0 + h, x0:x0 + w] = v
    return Y


def find(sums, W, H, bits=8, nframes=None, cap=16, **params):
    from amatsukaze_amd.api import logo_candidates_host
    return logo_candidates_host(sums, W, H, bits, nframes, cap, **params)


def rect(c):
    return c.imgx, c.imgy, c.w, c.h


def square_box(x0, y0, w, h, W, H):
    """edge pixels of a static square over moving noise: one pixel either side of its border, the frame's outer ring excluded"""
    return max(1, x0 - 1), max(1, y0 - 1), min(W - 2, x0 + w), min(H - 2, y0 + h)


def test_static_square_over_moving_noise_is_one_rectangle(lib):
    W, H, N = 96, 64, 48
    Y = put_square(noise_clip(N, W, H), 30, 20, 30, 20, 200)
    cands, n = find(LF.sums(Y, W, H), W, H, nframes=N)
    assert n == 1
    assert rect(cands[0]) == LF.rect_of_box(*square_box(30, 20, 30, 20, W, H), W, H)
    assert cands[0].coherence > 0.7 and cands[0].edge_pixels > 0
    # the same at 10 bits (samples x4, min_edge in 8-bit units): the same rectangle
    cands10, n10 = find(LF.sums(Y * 4, W, H), W, H, bits=10, nframes=N)
    assert n10 == 1 and rect(cands10[0]) == rect(cands[0])


def test_moving_noise_alone_gives_no_candidate(lib):
    W, H, N = 96, 64, 48
    assert find(LF.sums(noise_clip(N, W, H, seed=7, lo=0, amp=256), W, H), W, H, nframes=N) == ([], 0)
    assert find(LF.sums(noise_clip(N, W, H, seed=8), W, H), W, H, nframes=N) == ([], 0)
    # no frames at all: nothing to find
    assert find(np.zeros(2 * W * H, np.int64), W, H, nframes=0) == ([], 0)


def test_two_logos_are_ranked_by_score(lib):
    W, H, N = 128, 80, 40
    Y = noise_clip(N, W, H, seed=3)
    put_square(Y, 70, 40, 24, 20, 120)          # weak: contrast ~40
    put_square(Y, 10, 10, 24, 20, 220)          # strong: contrast ~140
    cands, n = find(LF.sums(Y, W, H), W, H, nframes=N)
    assert n == 2
    assert rect(cands[0]) == LF.rect_of_box(*square_box(10, 10, 24, 20, W, H), W, H)
    assert rect(cands[1]) == LF.rect_of_box(*square_box(70, 40, 24, 20, W, H), W, H)
    assert cands[0].score > cands[1].score > 0


@pytest.mark.parametrize("W,H", [(96, 64), (97, 65)])
def test_rectangles_at_frame_edges_and_corners(lib, W, H):
    """squares touching each edge and corner: the margin is clipped, the corner rounded down to even, the size up to even and cut
    back to a whole pair where an odd frame size ends it"""
    N = 40
    sw, sh = 20, 18
    spots = [(0, 0), (W - sw, 0), (0, H - sh), (W - sw, H - sh), (38, 0), (38, H - sh), (0, 23), (W - sw, 23)]
    for (x0, y0) in spots:
        Y = put_square(noise_clip(N, W, H, seed=x0 * 131 + y0), x0, y0, sw, sh, 210)
        for margin in (0, 3, 4):
            cands, n = find(LF.sums(Y, W, H), W, H, nframes=N, margin=margin, min_w=8, min_h=8)
            assert n == 1, (x0, y0, margin)
            r = rect(cands[0])
            assert r == LF.rect_of_box(*square_box(x0, y0, sw, sh, W, H), W, H, margin), (x0, y0, margin, r)
            assert r[0] % 2 == 0 and r[1] % 2 == 0 and r[2] % 2 == 0 and r[3] % 2 == 0
            assert r[0] + r[2] <= W and r[1] + r[3] <= H


def test_ties_are_broken_by_position(lib):
    """identical squares on a still background score exactly the same: ranked by (imgy, imgx), the same on every call"""
    W, H, N = 160, 120, 5
    Y = np.full((N, H, W), 60, np.int64)
    spots = [(100, 10), (20, 60), (20, 10), (100, 60), (60, 10)]
    for x0, y0 in spots:
        put_square(Y, x0, y0, 20, 20, 180)
    s = LF.sums(Y, W, H)
    cands, n = find(s, W, H, nframes=N)
    assert n == 5
    assert len({c.score for c in cands}) == 1
    want = sorted(LF.rect_of_box(*square_box(x0, y0, 20, 20, W, H), W, H) for x0, y0 in spots)
    assert [rect(c) for c in cands] == sorted(want, key=lambda r: (r[1], r[0]))
    for _ in range(3):
        assert find(s, W, H, nframes=N)[0] == cands


def test_cap_keeps_the_best_and_reports_the_total(lib):
    W, H, N = 160, 120, 40
    Y = noise_clip(N, W, H, seed=5)
    for i, (x0, y0) in enumerate([(10, 10), (60, 10), (110, 10), (10, 70), (60, 70)]):
        put_square(Y, x0, y0, 20, 20, 110 + 25 * i)
    s = LF.sums(Y, W, H)
    full, n = find(s, W, H, nframes=N, cap=16)
    assert n == 5 and len(full) == 5
    assert [c.score for c in full] == sorted((c.score for c in full), reverse=True)
    for cap in (0, 1, 3):
        got, total = find(s, W, H, nframes=N, cap=cap)
        assert total == 5 and got == full[:cap]


def test_size_limits(lib):
    W, H, N = 128, 96, 40
    Y = noise_clip(N, W, H, seed=9)
    put_square(Y, 10, 10, 8, 8, 220)             # smaller than 16 x 16
    put_square(Y, 40, 30, 80, 20, 220)           # wider than half the frame
    assert find(LF.sums(Y, W, H), W, H, nframes=N)[1] == 0
    cands, n = find(LF.sums(Y, W, H), W, H, nframes=N, min_w=4, min_h=4, max_w_frac=1.0)
    assert n == 2


def test_refused_arguments(lib):
    from amatsukaze_amd import binding
    from amatsukaze_amd.api import logo_find_params
    W, H = 16, 12
    s = np.zeros(2 * W * H, np.int64)
    out = (binding.LogoRect * 4)()
    n = C.c_int(-7)
    sp = s.ctypes.data_as(C.c_void_p)
    p = logo_find_params()
    call = lib.amtgpu_logofind_candidates_host
    assert call(sp, W, H, 8, 10, C.byref(p), out, 4, C.byref(n)) == 1 and n.value == 0
    assert call(sp, W, H, 8, 10, None, out, 4, C.byref(n)) == 1              # NULL params = defaults
    assert call(None, W, H, 8, 10, None, out, 4, C.byref(n)) == 0
    assert call(sp, W, H, 8, 10, None, out, 4, None) == 0
    assert call(sp, W, H, 8, 10, None, None, 4, C.byref(n)) == 0
    assert call(sp, W, H, 8, 10, None, None, 0, C.byref(n)) == 1             # nothing asked for: no output array needed
    for args in ((2, H, 8, 10), (W, 2, 8, 10), (W, H, 7, 10), (W, H, 17, 10), (W, H, 8, -1)):
        assert call(sp, *args, None, out, 4, C.byref(n)) == 0, args
    assert call(sp, W, H, 8, 10, None, out, -1, C.byref(n)) == 0
    for bad in (dict(min_coherence=1.5), dict(min_coherence=-0.1), dict(min_edge=-1.0), dict(join=-1), dict(margin=-1), dict(min_w=0),
                dict(min_h=0), dict(max_w_frac=0.0), dict(max_h_frac=1.5)):
        assert call(sp, W, H, 8, 10, C.byref(logo_find_params(**bad)), out, 4, C.byref(n)) == 0, bad
    with pytest.raises(TypeError):
        logo_find_params(no_such_field=1)


def test_default_parameters_are_documented_values(lib):
    from amatsukaze_amd.api import logo_find_params
    p = logo_find_params()
    assert (p.min_coherence, p.min_edge, p.join, p.margin, p.min_w, p.min_h, p.max_w_frac, p.max_h_frac) == (pytest.approx(0.6), 3.0, 4, 4, 16, 16, 0.5, 0.5)
