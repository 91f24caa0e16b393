"""The tile kernels' frame offsets at their corners, against the CPU oracle (like tests/test_gpu_eval_shapes.py).

A wave of the scan (pair) kernel or of the linear analysis kernel forms the byte offset of a staging unit's row as
(imgy + row0 + y * row_step) * pitch_bytes with 24-bit multiplies (csrc/eval_tiles.hpp mul24): the operands are small, the product is
not.  Geometries, each at 8 and 10 bits, with the smallest logo AMTAnalyzeLogo takes (6 x 12: its field logos are 6 x 6, the tile kernels'
minimum is 6 x 5) and with a 256 x 128 one:

  far_rows       pitch 8192 bytes, 2304 rows, the logo from row 2100 on: every row offset the kernels form is beyond 2^24
  origin         the rectangle at imgx = imgy = 0
  last_sample    the rectangle ends on the last sample of a plane without row padding
  odd_pitch      a pitch that is no multiple of 4 samples (354), the plane's base one sample into its allocation: a 16-bit plane
                 that is 2-byte aligned only

Per case: the scan's records are the oracle's bytes and come from the pair kernel; the exact analysis records are the oracle's bytes;
the linear mode's scores -- from the linear kernel -- are within amtgpu_analyze_error_bound of the oracle's; its fades are the exact mode's
bytes."""
import ctypes as C

import numpy as np
import pytest

import amt_synth as S
from amtlib import Oracle, _ptr
from test_gpu_parity import gpu, oracle_eval_logos  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

N = 3
GEOMETRIES = {
    # name: (W, H, pitch in BYTES or None = width, (imgx, imgy) as a function of the logo size, base offset in samples)
    "far_rows": (352, 2304, 8192, lambda lw, lh: (64, 2100), 0),
    "origin": (352, 240, None, lambda lw, lh: (0, 0), 0),
    "last_sample": (352, 240, None, lambda lw, lh: (352 - lw, 240 - lh), 0),
    "odd_pitch": (352, 240, "odd", lambda lw, lh: (226 if lw < 100 else 94, 22), 1),      # (origins even, 2 mod 4)
}
LOGOS = {"tiny": (6, 12), "hd": (256, 128)}


def tiny_logo(lw, lh):
    """S.make_logo keeps an 8-pixel ring of every logo clear: nothing is left of a logo this small.  A dense pattern of alpha 0.08 .. 0.5,
    laid out as make_logo's (aY, bY, aU, bU, aV, bV: AMTLogo.hpp:204-212)."""
    yy, xx = np.mgrid[0:lh, 0:lw]
    alpha = (0.08 + 0.07 * ((xx * 3 + yy * 5) % 7)).astype(np.float64)
    cY, cC = 235.0 / 255.0, 128.0 / 255.0
    aY = (1.0 / (1.0 - alpha)).astype(np.float32)
    bY = (-alpha * cY / (1.0 - alpha)).astype(np.float32)
    alphaUV = alpha.reshape(lh // 2, 2, lw // 2, 2).mean(axis=(1, 3))
    aC = (1.0 / (1.0 - alphaUV)).astype(np.float32)
    bC = (-alphaUV * cC / (1.0 - alphaUV)).astype(np.float32)
    return np.concatenate([aY.ravel(), bY.ravel(), aC.ravel(), bC.ravel(), aC.ravel(), bC.ravel()]).astype(np.float32), alpha, alphaUV


def kernels_used(ctx):
    return sorted(k for k, (calls, _) in ctx.profile_report().items() if calls)


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("logo_kind", sorted(LOGOS))
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_tile_kernels_at_offset_corners(gpu, geometry, logo_kind, bits):
    from amatsukaze_amd import AMTAnalyzeLogo, AMTEraseLogo, DeviceClip, Logo, LogoFrame
    torch, ctx, dev = gpu["torch"], gpu["ctx"], gpu["dev"]
    W, H, pitch_bytes, origin, base_off = GEOMETRIES[geometry]
    LW, LH = LOGOS[logo_kind]
    X, Y0 = origin(LW, LH)
    es = 1 if bits <= 8 else 2
    pitch = W if pitch_bytes is None else (W + 2 if pitch_bytes == "odd" else pitch_bytes // es)
    assert pitch >= W and (geometry != "odd_pitch" or pitch % 4 != 0)
    if geometry == "far_rows":
        assert (Y0 * pitch * es) > (1 << 24) and pitch * es == 8192
    data, alpha, alphaUV = tiny_logo(LW, LH) if logo_kind == "tiny" else S.make_logo(LW, LH)
    clip = S.make_clip_np(N, W, H, 0x5EED0077, alpha, alphaUV, X, Y0, bits=bits, period=4, fade=2, flat_every=3, pitchY=pitch, pitchUV=W // 2)
    Y = clip["Y"]
    assert Y.shape == (N, H, pitch)
    tdt, ndt = (torch.uint8, np.uint8) if bits <= 8 else (torch.int16, np.int16)
    # the plane `base_off` samples into its allocation (torch allocations are 256-byte aligned: the 16-bit plane is then 2-byte aligned only)
    buf = torch.zeros(Y.size + base_off, dtype=tdt, device=dev)
    dY = buf[base_off:].view(N, H, pitch)
    dY.copy_(torch.from_numpy(Y.view(ndt)))
    assert dY.data_ptr() % 4 == (base_off * es) % 4
    dU, dV = (torch.from_numpy(clip[k].view(ndt)).to(dev) for k in "UV")
    dclip = DeviceClip(dY, dU, dV, width=W, height=H, bits=bits)
    logo = Logo.from_planes(ctx, data, LW, LH, W, H, X, Y0)
    orc = Oracle()
    lo = orc.make_logo(data, LW, LH, W, H, X, Y0)
    d, t, b = oracle_eval_logos(orc, lo)
    want_scan = np.zeros(N * 2, np.float32)
    orc.lib.orc_logoframe_scan((C.c_void_p * 1)(d), 1, _ptr(Y), Y.strides[0], Y.shape[2], bits, W, H, N, _ptr(want_scan))
    want = np.zeros(N * 33, np.float32)
    orc.lib.orc_analyze_frames(d, t, b, _ptr(Y), Y.strides[0], Y.shape[2], bits, N, _ptr(want))
    want = want.reshape(N, 33)
    assert np.isfinite(want).all() and np.isfinite(want_scan).all()

    ctx.profile(True)
    try:
        lf = LogoFrame(ctx, [logo], 0.35)
        lf.scanFrames(dclip)
        got_scan = lf.evalResults
        used_scan = kernels_used(ctx)
    finally:
        ctx.profile(False)
    assert used_scan == ["logo_eval_pair_kernel.scan"], used_scan
    assert got_scan.reshape(-1).tobytes() == want_scan.tobytes()

    exact = AMTAnalyzeLogo(ctx, logo, 0.35).analyze(dclip)
    assert exact.tobytes() == want.tobytes()
    an = AMTAnalyzeLogo(ctx, logo, 0.35, mode="linear")
    ctx.profile(True)
    try:
        got = an.analyze(dclip)
        used = kernels_used(ctx)
    finally:
        ctx.profile(False)
    assert any(k.startswith("logo_eval_linear_kernel") for k in used), used
    err = np.abs(got - want)
    scale = max(1.0, float(np.abs(want).max()))
    for k in range(3):
        bound = an.error_bound(k, bits) * scale
        print(f"{geometry} {logo_kind} {bits}: group {k} max error {float(err[:, 11 * k:11 * k + 11].max()):.3e}, bound {bound:.3e}, refined {an.last_refined()}")
        assert err[:, 11 * k:11 * k + 11].max() <= bound
    er = AMTEraseLogo(ctx, logo, "", 0, 16)
    assert er.calc_fades(got, N).tobytes() == er.calc_fades(exact, N).tobytes()
