"""The scan kernel on taps that carry DeintY's 0.25 (csrc/eval_tile_stage.h Quad, EvalEngine::stage4_eligible), against the CPU oracle.

For its (deinterlaced) logos the scan's pair kernel stages the [1 2 1] row sums unscaled -- {4 s, 4 bg} in the tile planes -- on taps the
host scaled by 0.25; only the bin select sees the factor.  The records must be the bits they were.  Each case compares the scan's
records and the exact analysis' with the oracle's bytes and the linear analysis mode's with the exact mode's (bytes on the frames its
guard hands to the exact kernel, 1e-4 otherwise) -- the linear kernel shares the staging code and keeps the scaled-sample form.
What is covered here and nowhere else:

  * a 24 x 12 logo with every interior pixel in the mask (maskratio 1): the windows of the pixels in rows 2 and h - 3 reach the
    logo's first and last row, which DeintY copies -- unblended rows of a blended logo go through the same unscaled path with bias 0;
  * 8, 10 and 16 bits, with an all-zero frame, a frame of nothing but the sample maximum (65535 at 16 bits: the largest [1 2 1] sum,
    4 * 65535 + 2) and a frame of noise in front of three frames of a picture with the logo fading in;
  * the rectangle at an even and at an odd origin;
  * a logo with coefficients (and through them taps) below the eligibility limit: the engine keeps plain taps and runs the kernel's
    ldexp form -- asserted from the kernel's name -- and still equals the oracle;
  * a logo with |a| + |b| just below the magnitude limit of 8192, where 4 bg is largest.
"""
import ctypes as C

import numpy as np
import pytest

from amtlib import Oracle, _ptr
from test_gpu_parity import gpu, oracle_eval_logos  # noqa: F401  (fixture + helper)
from test_gpu_linear_offsets import kernels_used, tiny_logo

pytestmark = pytest.mark.gpu

W, H, LW, LH = 96, 64, 24, 12
RATIO = 1.0                                # every interior pixel: rows 2 and LH - 3 are in the mask, their windows reach rows 0 and LH - 1


def make_frames(bits, x0, y0, alpha, seed=0x5EED0095):
    """[zeros, all maxv, noise, picture with the logo at 0 / 50 / 100 %]"""
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(seed + bits)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (16.0 + ((xx * 7 + yy * 13) % 180) + rng.integers(0, 6, (H, W))) / 255.0 * maxv
    frames = [np.zeros((H, W)), np.full((H, W), float(maxv)), rng.integers(0, maxv + 1, (H, W)).astype(np.float64)]
    for f in (0.0, 0.5, 1.0):
        p = base.copy()
        r = p[y0:y0 + LH, x0:x0 + LW]
        p[y0:y0 + LH, x0:x0 + LW] = r * (1.0 - alpha * f) + alpha * f * (235.0 / 255.0 * maxv)
        frames.append(p)
    Y = np.clip(np.rint(np.stack(frames)), 0, maxv).astype(np.uint8 if bits <= 8 else np.uint16)
    assert Y[1].min() == maxv and Y[0].max() == 0
    return Y


def device_clip(gpu, Y, bits):
    from amatsukaze_amd import DeviceClip
    torch = gpu["torch"]
    tdt, ndt = (torch.uint8, np.uint8) if bits <= 8 else (torch.int16, np.int16)
    n = Y.shape[0]
    mid = np.full((n, H // 2, W // 2), 1 << (bits - 1), Y.dtype)
    return DeviceClip(*(torch.from_numpy(p.view(ndt)).to(gpu["dev"]).to(tdt) for p in (Y, mid, mid)), width=W, height=H, bits=bits)


def run_case(gpu, data, bits, x0, y0, Y, pair_kernel, linear_kernel=True):
    """scan records and exact analysis records: the oracle's bytes; linear analysis: see the module's text.  Returns the oracle's records."""
    from amatsukaze_amd import AMTAnalyzeLogo, AMTEraseLogo, Logo, LogoFrame
    ctx = gpu["ctx"]
    n = Y.shape[0]
    dclip = device_clip(gpu, Y, bits)
    logo = Logo.from_planes(ctx, data, LW, LH, W, H, x0, y0)
    orc = Oracle()
    lo = orc.make_logo(data, LW, LH, W, H, x0, y0)
    d, t, b = oracle_eval_logos(orc, lo, RATIO)
    want_scan = np.zeros(n * 2, np.float32)
    orc.lib.orc_logoframe_scan((C.c_void_p * 1)(d), 1, _ptr(Y), Y.strides[0], Y.shape[2], bits, W, H, n, _ptr(want_scan))
    want = np.zeros(n * 33, np.float32)
    orc.lib.orc_analyze_frames(d, t, b, _ptr(Y), Y.strides[0], Y.shape[2], bits, n, _ptr(want))
    want = want.reshape(n, 33)

    ctx.profile(True)
    try:
        lf = LogoFrame(ctx, [logo], RATIO)
        lf.scanFrames(dclip)
        got_scan = lf.evalResults
        used_scan = kernels_used(ctx)
    finally:
        ctx.profile(False)
    assert used_scan == [pair_kernel], used_scan
    assert got_scan.reshape(-1).tobytes() == want_scan.tobytes()

    exact = AMTAnalyzeLogo(ctx, logo, RATIO).analyze(dclip)
    assert exact.tobytes() == want.tobytes()

    an = AMTAnalyzeLogo(ctx, logo, RATIO, mode="linear")
    ctx.profile(True)
    try:
        got = an.analyze(dclip)
        used = kernels_used(ctx)
    finally:
        ctx.profile(False)
    # (window values beyond 2^30 / 16 -- the magnitude limit at 16 bits -- are outside the linear kernel's fixed point: run_linear hands the
    #  whole batch to the exact kernel)
    assert any(k.startswith("logo_eval_linear_kernel.") for k in used) == linear_kernel, used
    err = np.abs(got - want)
    scale = max(1.0, float(np.nanmax(np.abs(want))))
    print(f"bits {bits} origin ({x0}, {y0}): linear max error {float(np.nanmax(err)):.3e}, refined {an.last_refined()} of {n}")
    assert np.isfinite(want).all()
    assert (err <= 1e-4 * np.maximum(1.0, np.abs(want))).all(), float(err.max())
    for k in range(3):                       # (and inside the library's own bound, whatever the logo)
        assert np.nanmax(err[:, 11 * k:11 * k + 11]) <= an.error_bound(k, bits) * scale
    # the frames the guard handed to the exact kernel carry its bytes
    same = (got.view(np.uint32) == exact.view(np.uint32)).all(axis=1)
    assert int(same.sum()) >= an.last_refined(), (int(same.sum()), an.last_refined())
    er = AMTEraseLogo(ctx, logo, "", 0, 16)
    assert er.calc_fades(got, n).tobytes() == er.calc_fades(exact, n).tobytes()
    return want_scan, want


@pytest.mark.parametrize("origin", [(40, 20), (41, 21)], ids=["even_origin", "odd_origin"])
@pytest.mark.parametrize("bits", [8, 10, 16])
def test_unscaled_staging_equals_the_oracle(gpu, bits, origin):
    x0, y0 = origin
    data, alpha, _ = tiny_logo(LW, LH)
    Y = make_frames(bits, x0, y0, alpha)
    want_scan, want = run_case(gpu, data, bits, x0, y0, Y, "logo_eval_pair_kernel.scan")
    assert np.abs(want_scan).max() > 0 and np.abs(want).max() > 0


@pytest.mark.parametrize("bits", [8, 16])
def test_logo_below_the_eligibility_limit_takes_the_ldexp_form(gpu, bits):
    """An 8 x 8 block of the logo with a = 1 and b a few 1e-41 (denormal): nonzero coefficients below 2^-64, and -- where a window lies
    inside the block -- nonzero taps below 2^-124, whose quarter would lose bits.  The engine keeps plain taps."""
    data, alpha, _ = tiny_logo(LW, LH)
    a = data[:LW * LH].reshape(LH, LW)
    b = data[LW * LH:2 * LW * LH].reshape(LH, LW)
    yy, xx = np.mgrid[2:10, 8:16]
    a[2:10, 8:16] = 1.0
    b[2:10, 8:16] = (-(1 + (xx * 3 + yy * 5) % 7) * 1e-41).astype(np.float32)
    assert (b[2:10, 8:16] != 0).all() and np.abs(b[2:10, 8:16]).max() < 2.0 ** -124
    Y = make_frames(bits, 40, 20, alpha)
    run_case(gpu, data, bits, 40, 20, Y, "logo_eval_pair_ldexp_kernel.scan")


@pytest.mark.parametrize("bits", [8, 16])
def test_logo_at_the_magnitude_limit(gpu, bits):
    """Three vertically adjacent pixels with a = 8100, b = -90 (|a| + |b| = 8190 < 8192 survives DeintY's [1 2 1] of the coefficients):
    4 bg reaches 4 * 8190 * maxv, 2.1e9 at 16 bits, and the scaled mean clamps at 1020 where the plain one clamped at 255.  Scaled taps;
    scan and exact analysis are the oracle's bytes, the linear mode as for any logo."""
    data, alpha, _ = tiny_logo(LW, LH)
    a = data[:LW * LH].reshape(LH, LW)
    b = data[LW * LH:2 * LW * LH].reshape(LH, LW)
    a[4:7, 11] = 8100.0
    b[4:7, 11] = -90.0
    Y = make_frames(bits, 40, 20, alpha)
    run_case(gpu, data, bits, 40, 20, Y, "logo_eval_pair_kernel.scan", linear_kernel=bits <= 8)
