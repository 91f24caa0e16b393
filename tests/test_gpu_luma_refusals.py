"""What the entry points of the passes that read the Y plane alone refuse, and what they let through without looking: the logo evaluation
(AMTAnalyzeLogo, LogoFrame), the logo finder and the frame metrics.  Each case pins the return value and the context's message; every call
is refused, or returns, before a kernel is launched, so nothing here depends on what a kernel computes.

The clip is one 10-bit frame of zeros, just large enough for the smallest logo of logo_sets that AMTAnalyzeLogo takes (w >= 6, h >= 12).
An odd byte stride is harmless with one frame: the stride is only ever multiplied by a frame index, and frame 0 is the only one."""
import ctypes as C

import pytest

import logo_sets as LS
from test_gpu_parity import gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

LW, LH = LS.WIDE_MIXED[1][:2]          # 36 x 60
W, H, BITS = LW, LH, 10
PITCH = W
STRIDE = 2 * H * PITCH                 # bytes
ODD = STRIDE + 1
ODD_STRIDE = "frame stride not a multiple of the sample size"


@pytest.fixture(scope="module")
def env(gpu):
    from amatsukaze_amd import Logo
    torch, ctx = gpu["torch"], gpu["ctx"]
    logo = Logo.from_planes(ctx, LS.logo_data(LS.WIDE_MIXED[1]), LW, LH, W, H, 0, 0)
    Y = torch.zeros((1, H, PITCH), dtype=torch.int16, device=gpu["dev"])
    return dict(ctx=ctx, lib=ctx.lib, logo=logo, Y=Y, pY=C.c_void_p(Y.data_ptr()), torch=torch, dev=gpu["dev"])


def message(env):
    return env["lib"].amtgpu_last_error(env["ctx"].h).decode(errors="replace")


def refused(env, ret, text):
    assert ret == 0 and message(env) == text, (ret, message(env))


@pytest.mark.parametrize("mode", ["exact", "linear", "monitored"])
def test_analyze_batch(env, mode):
    from amatsukaze_amd import AMTAnalyzeLogo
    an = AMTAnalyzeLogo(env["ctx"], env["logo"], LS.MASKRATIO, mode=mode)
    out = env["torch"].zeros((1, 33), dtype=env["torch"].float32, device=env["dev"])
    call = lambda stride, bits, n: env["lib"].amtgpu_analyze_batch(an.h, env["pY"], stride, PITCH, bits, n, C.c_void_p(out.data_ptr()))
    refused(env, call(ODD, BITS, 1), ODD_STRIDE)
    assert call(ODD, BITS, 0) == 1                      # an empty batch: its stride is never judged
    for bits in (7, 17):
        refused(env, call(STRIDE, bits, 1), "[AMTAnalyzeLogo] Unsupported pixel format")


def test_logoframe_scan_batch(env):
    from amatsukaze_amd import LogoFrame
    lf = LogoFrame(env["ctx"], [env["logo"]], LS.MASKRATIO)
    lf.begin(W, H, BITS, 1)
    call = lambda stride, first, n: env["lib"].amtgpu_logoframe_scan_batch(lf.h, env["pY"], stride, PITCH, first, n)
    refused(env, call(ODD, 0, 1), ODD_STRIDE)
    assert call(ODD, 0, 0) == 1
    for stride in (STRIDE, ODD):                        # the range check comes first
        refused(env, call(stride, 0, 2), "frame range outside the clip")
        refused(env, call(stride, 1, 1), "frame range outside the clip")


def test_logofind_add_batch(env):
    lib = env["lib"]
    h = lib.amtgpu_logofind_create(env["ctx"].h, W, H, BITS)
    assert h
    try:
        call = lambda p, stride, pitch, n: lib.amtgpu_logofind_add_batch(h, p, stride, pitch, n)
        below = "[LogoFind] pitch below the width or negative frame stride"
        refused(env, call(env["pY"], STRIDE, PITCH, -1), "[LogoFind] negative frame count")
        refused(env, call(None, STRIDE, PITCH, 1), "[LogoFind] null frame pointer")
        refused(env, call(env["pY"], STRIDE, W - 1, 1), below)
        refused(env, call(env["pY"], -2, PITCH, 1), below)
        # several faults at once: the earlier check wins
        refused(env, call(None, STRIDE, PITCH, -1), "[LogoFind] negative frame count")
        refused(env, call(None, -2, W - 1, 1), "[LogoFind] null frame pointer")
        assert call(None, STRIDE, PITCH, 0) == 1        # an empty batch is not looked at
        assert lib.amtgpu_logofind_nframes(h) == 0
    finally:
        lib.amtgpu_logofind_destroy(h)


def test_framestats_batch_empty(env):
    lib = env["lib"]
    h = lib.amtgpu_framestats_create(env["ctx"].h, W, H, BITS)
    assert h
    try:
        out = env["torch"].zeros(8, dtype=env["torch"].int64, device=env["dev"])
        assert lib.amtgpu_framestats_batch(h, env["pY"], ODD, PITCH, None, 0, C.c_void_p(out.data_ptr())) == 1
    finally:
        lib.amtgpu_framestats_destroy(h)
