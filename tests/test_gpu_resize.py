"""The resize on the GPU (amtgpu_resize_*, Resizer) against its numpy restatement (tests/resize_ref.py, which
tests/test_resize_host.py holds against the C++ plan and against the continuous definition): every destination container of the three
planes, byte for byte, with sentinel guard containers in front of, between and behind the rows and frames; both lane forms and both
container sizes; every K the register forms and the table walk take; planted constants and step edges; rounds; and every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import resize_ref as R
from test_gpu_temporal_nr import Buf, check_against, download, sentinel_buf, upload

pytestmark = pytest.mark.gpu


def aligned_layouts(sw, sh, dw, dh, bits):
    """(source, destination) layouts on which both stages take their 16-byte form: every row of every plane 16-byte aligned; the two
    differ in pitches and strides, and the destination has guard containers in front of, between and behind its frames"""
    es = 1 if bits <= 8 else 2
    up = lambda v: (v * es + 15) // 16 * 16 // es
    src = dict(pitch=(up(sw), up(sw // 2)), tight_end=True)
    dst = dict(pitch=(up(dw) + 16 // es, up(dw // 2) + 32 // es), gap=(32 // es, 48 // es), off=(16 // es, 32 // es, 16 // es))
    return src, dst


def narrow_layouts(sw, sh, dw, dh, bits):
    """plane bases one container off and pitches that are no multiple of 16 bytes: the container-by-container form"""
    src = dict(pitch=(sw + 1, sw // 2 + 2), gap=(3, 1), off=(1, 1, 1), tight_end=True)
    dst = dict(pitch=(dw + 3, dw // 2 + 1), gap=(1, 5), off=(1, 3, 1))
    return src, dst


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    ctx = Context(0)
    yield ctx, torch
    ctx.close()


@functools.lru_cache(maxsize=None)
def noise_case(n, sw, sh, dw, dh, bits, kernel="blackman"):
    """(planes, the reference's planes) of seeded noise over the depth's whole range; computed once, read-only"""
    planes = R.make_clip(n, sw, sh, bits, np.random.default_rng(sw * 131 + sh * 7 + dw * 3 + dh + bits))
    want = R.resize_clip(planes, dw, dh, bits, kernel)
    for a in planes + want:
        a.setflags(write=False)
    return planes, want


def run_resize(gpu, what, planes, bits, dst_size, layouts, want, kernel="blackman", max_scratch_bytes=None, taps=None):
    """resizes the whole clip in one call and compares every destination container; the sources must stay as they were.  Returns the
    destination's flat buffers as they came back"""
    from amatsukaze_amd import Resizer
    ctx, torch = gpu
    n, sh, sw = planes[0].shape
    dw, dh = dst_size
    sl, dl = layouts(sw, sh, dw, dh, bits)
    src_host = Buf(n, sw, sh, bits, **sl).put(planes)
    dst_host = sentinel_buf(n, dw, dh, bits, dl)
    src, src_flat = upload(gpu, src_host)
    dst, dst_flat = upload(gpu, dst_host)
    rz = Resizer(ctx, (sw, sh), (dw, dh), bits, kernel=kernel, taps=taps, max_scratch_bytes=max_scratch_bytes)
    try:
        assert rz.run(src, dst) == n
        for plane, (S_w, S_h, D_w, D_h) in enumerate(((sw, sh, dw, dh), (sw // 2, sh // 2, dw // 2, dh // 2))):
            for axis, (S, D) in enumerate(((S_w, D_w), (S_h, D_h))):
                K, start, coeff = rz.program(plane, axis)
                rK, rstart, rC = R.program(S, D, kernel, taps)
                assert K == rK and np.array_equal(start, rstart) and np.array_equal(coeff, rC), (what, "program", plane, axis)
    finally:
        rz.close()
    torch.cuda.synchronize()
    got = download(dst_host, dst_flat)
    check_against(what, dst_host, got, want)
    for g, a in zip(download(src_host, src_flat), src_host.flat):
        assert np.array_equal(g, a), (what, "the source changed")
    return got


# ---- shapes ----
@pytest.mark.parametrize("layouts", [aligned_layouts, narrow_layouts], ids=["aligned", "narrow"])
@pytest.mark.parametrize("bits", [8, 10])
def test_three_to_two(gpu, bits, layouts):
    # 48x36 -> 32x24: K 12 in luma, chroma planes 24x18 -> 16x12
    assert R.program(48, 32)[0] == 12 and R.program(18, 12)[0] == 12
    planes, want = noise_case(2, 48, 36, 32, 24, bits)
    run_resize(gpu, ("3:2", bits), planes, bits, (32, 24), layouts, want)


@pytest.mark.parametrize("layouts", [aligned_layouts, narrow_layouts], ids=["aligned", "narrow"])
@pytest.mark.parametrize("bits", [8, 10])
def test_an_irregular_ratio_with_three_waves_and_a_tail(gpu, bits, layouts):
    # 272x48 -> 182x34: a luma row is three runs of output columns, the last of 54; a chroma row has 91 columns
    assert 182 - 2 * 64 == 54 and R.program(272, 182)[0] == 12
    planes, want = noise_case(2, 272, 48, 182, 34, bits)
    run_resize(gpu, ("272 -> 182", bits), planes, bits, (182, 34), layouts, want)


@pytest.mark.parametrize("bits", [8, 10])
def test_upscaling_has_coefficients_above_one(gpu, bits):
    K, _, Cf = R.program(32, 50)
    assert K == 8 and int(Cf.max()) == 17723 and int(Cf.min()) < 0
    planes, want = noise_case(2, 32, 24, 50, 40, bits)
    run_resize(gpu, ("32x24 -> 50x40", bits), planes, bits, (50, 40), aligned_layouts, want)


@pytest.mark.parametrize("layouts", [aligned_layouts, narrow_layouts], ids=["aligned", "narrow"])
@pytest.mark.parametrize("bits", [8, 10])
def test_equal_sizes_copy(gpu, bits, layouts):
    planes, want = noise_case(2, 64, 32, 64, 32, bits)
    for p, w in zip(planes, want):
        assert np.array_equal(p, w)                                 # the reference itself: a single 16384 per row
    run_resize(gpu, ("64x32 -> 64x32", bits), planes, bits, (64, 32), layouts, planes)


@pytest.mark.parametrize("layouts", [aligned_layouts, narrow_layouts], ids=["aligned", "narrow"])
@pytest.mark.parametrize("bits", [8, 10])
def test_windows_as_wide_as_the_plane(gpu, bits, layouts):
    # 16x8 -> 8x4: K = S = 16 in luma rows; in chroma 8 -> 4 folds K0 = 16 into K = S = 8, and 4 -> 2 into 4
    assert R.program(16, 8)[0] == 16 and R.program(8, 4)[0] == 8 and R.program(4, 2)[0] == 4
    planes, want = noise_case(3, 16, 8, 8, 4, bits)
    run_resize(gpu, ("16x8 -> 8x4", bits), planes, bits, (8, 4), layouts, want)


def test_the_table_walk_takes_windows_above_16_taps(gpu):
    # 160 -> 32 has K 40: more than the register forms hold; chroma 80 -> 16 too
    assert R.program(160, 32)[0] == 40 and R.program(80, 16)[0] == 40 and R.program(24, 16)[0] == 12
    for bits in (8, 10):
        planes, want = noise_case(2, 160, 24, 32, 16, bits)
        run_resize(gpu, ("160x24 -> 32x16", bits), planes, bits, (32, 16), aligned_layouts, want)


@pytest.mark.parametrize("kernel, K", [("lanczos", 9), ("bilinear", 3)])
def test_the_other_kernels(gpu, kernel, K):
    assert R.program(48, 32, kernel)[0] == K
    planes, want = noise_case(2, 48, 36, 32, 24, 10, kernel)
    assert not np.array_equal(want[0], noise_case(2, 48, 36, 32, 24, 10)[1][0])
    run_resize(gpu, kernel, planes, 10, (32, 24), aligned_layouts, want, kernel=kernel)


# ---- planted inputs ----
@pytest.mark.parametrize("bits", [8, 10, 16])
def test_constant_planes_stay_constant(gpu, bits):
    maxv = (1 << bits) - 1
    dt = np.uint8 if bits <= 8 else np.uint16
    levels = np.array([0, 1, maxv], dt)
    planes = tuple(np.broadcast_to(levels[:, None, None], (3, h, w)).copy() for h, w in ((36, 48), (18, 24), (18, 24)))
    want = tuple(np.broadcast_to(levels[:, None, None], (3, h, w)).copy() for h, w in ((24, 32), (12, 16), (12, 16)))
    for a, b in zip(R.resize_clip(planes, 32, 24, bits), want):
        assert np.array_equal(a, b)                                 # sum(C) = 16384
    for layouts in (aligned_layouts, narrow_layouts):
        run_resize(gpu, ("constants", bits), planes, bits, (32, 24), layouts, want)


@pytest.mark.parametrize("direction", ["vertical edge", "horizontal edge"])
def test_step_edges_at_16_bits_reach_both_clamps(gpu, direction):
    bits, maxv = 16, 65535
    def edge(h, w):
        a = np.zeros((2, h, w), np.uint16)
        if direction == "vertical edge":
            a[0, :, w // 2:] = maxv
            a[1, :, :w // 2 - 3] = maxv
        else:
            a[0, h // 2:, :] = maxv
            a[1, :h // 2 - 1, :] = maxv
        return a
    planes = (edge(36, 48), edge(18, 24), edge(18, 24))
    # the unclamped sums of the stage that crosses the edge leave 0 .. maxv on both sides, and the largest one is the plan's bound
    K, start, Cf = R.program(48, 32) if direction == "vertical edge" else R.program(36, 24)
    line = planes[0][0, 0, :].astype(np.int64) if direction == "vertical edge" else planes[0][0, :, 0].astype(np.int64)
    acc = (line[start[:, None] + np.arange(K)[None, :]] * Cf).sum(axis=1)
    assert acc.min() < 0 and acc.max() > maxv * 16384 and acc.max() + 8192 < 2 ** 31
    want = R.resize_clip(planes, 32, 24, bits)
    assert int(want[0].min()) == 0 and int(want[0].max()) == maxv
    for layouts in (aligned_layouts, narrow_layouts):
        run_resize(gpu, direction, planes, bits, (32, 24), layouts, want)


# ---- rounds ----
def test_rounds_of_one_frame_give_the_bytes_of_the_default(gpu):
    from amatsukaze_amd import AmtError, Resizer
    ctx, _ = gpu
    bits = 10
    planes, want = noise_case(3, 48, 36, 32, 24, bits)
    # one frame's intermediate: rows of the destination's width rounded up to 16 bytes, the source's height of them, for three planes
    one = 64 * 36 + 2 * 32 * 18
    whole = run_resize(gpu, "default scratch", planes, bits, (32, 24), aligned_layouts, want)
    rounds = run_resize(gpu, "one frame per round", planes, bits, (32, 24), aligned_layouts, want, max_scratch_bytes=one)
    pairs = run_resize(gpu, "two frames, then one", planes, bits, (32, 24), aligned_layouts, want, max_scratch_bytes=2 * one + 17)
    for a, b, c in zip(whole, rounds, pairs):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    with pytest.raises(AmtError, match="below one frame's intermediate"):
        Resizer(ctx, (48, 36), (32, 24), bits, max_scratch_bytes=one - 1)


# ---- refusals ----
def test_refusals_launch_nothing(gpu):
    from amatsukaze_amd import AmtError, DeviceSurfaces, Resizer, binding
    ctx, torch = gpu
    N, sw, sh, dw, dh, bits = 3, 48, 36, 32, 24, 8
    planes, want = noise_case(N, sw, sh, dw, dh, bits)
    sl, dl = aligned_layouts(sw, sh, dw, dh, bits)
    src_host = Buf(N, sw, sh, bits, **sl).put(planes)
    src, src_flat = upload(gpu, src_host)
    dst_host = sentinel_buf(N, dw, dh, bits, dl)
    dst, dst_flat = upload(gpu, dst_host)
    s, t = src.ref(), dst.ref()

    def changed(desc, **kw):
        c = binding.Surfaces()
        C.memmove(C.byref(c), C.byref(desc), C.sizeof(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    for args, words in ((((0, 36), (32, 24), 8), "even and positive"), (((48, 36), (31, 24), 8), "even and positive"), (((48, 36), (32, 24), 7), "bits must be 8..16"),
                        (((48, 36), (32, 24), 17), "bits must be 8..16"), (((4096, 36), (2, 24), 8), "does not fit a wave's staging region")):
        with pytest.raises(AmtError, match=words):
            Resizer(ctx, *args)
    with pytest.raises(AmtError, match="kernel is one of"):
        Resizer(ctx, (48, 36), (32, 24), 8, kernel="bicubic")
    assert not ctx.lib.amtgpu_resize_create(ctx.h, 48, 36, 32, 24, 8, 3, 0, 0) and b"AMTGPU_RESIZE_" in ctx.lib.amtgpu_last_error(ctx.h)
    assert not ctx.lib.amtgpu_resize_create(ctx.h, 48, 36, 32, 24, 8, 0, 65, 0) and b"taps" in ctx.lib.amtgpu_last_error(ctx.h)

    rz = Resizer(ctx, (sw, sh), (dw, dh), bits)
    rz10 = Resizer(ctx, (sw, sh), (dw, dh), 10)                     # for descriptors that claim 10 bits: MSB alignment needs more than 8

    def call(s_, t_, n, r_=None):
        r = ctx.lib.amtgpu_resize_run((r_ or rz).h, C.byref(s_), C.byref(t_), n)
        return r, ctx.lib.amtgpu_last_error(ctx.h).decode(errors="replace")

    last_src_byte = s.Y + s.strideY * (N - 1) + (sh - 1) * s.pitchY + sw - 1
    cases = {
        "interleaved source": (changed(s, interleaved=1), t, N, "source: planar, LSB-aligned planes only"),
        "interleaved destination": (s, changed(t, interleaved=1), N, "destination: planar, LSB-aligned planes only"),
        "MSB-aligned source": (changed(s, bits=10, msb_aligned=1), changed(t, bits=10), N, "source: planar, LSB-aligned planes only", rz10),
        "MSB-aligned destination": (changed(s, bits=10), changed(t, bits=10, msb_aligned=1), N, "destination: planar, LSB-aligned planes only", rz10),
        "unequal bits": (s, changed(t, bits=10), N, "destination: 10 bits, the resizer was created for 8"),
        "both of another depth": (changed(s, bits=10), changed(t, bits=10), N, "source: 10 bits, the resizer was created for 8"),
        "source pitch below the row": (changed(s, pitchY=sw - 2), t, N, "source: pitch smaller than the row"),
        "destination chroma pitch below the row": (s, changed(t, pitchUV=dw // 2 - 1), N, "destination: pitch smaller than the row"),
        "negative source stride": (changed(s, strideY=-s.strideY), t, N, "source: negative frame stride"),
        "negative destination chroma stride": (s, changed(t, strideUV=-t.strideUV), N, "destination: negative frame stride"),
        "overlapping destination frames": (s, changed(t, strideY=(dh - 1) * t.pitchY + dw - 1), 2, "destination frames overlap each other"),
        "destination is the source": (s, changed(s), N, "overlaps the source's"),
        "destination luma inside the source's chroma": (s, changed(t, Y=s.U), 1, "overlaps the source's"),
        "destination one byte into the source": (s, changed(t, V=last_src_byte), N, "overlaps the source's"),
        "negative frame count": (s, t, -1, "negative frame count"),
        "null plane": (changed(s, V=None), t, N, "null surface plane"),
    }
    for what, (s_, t_, n, words, *other) in cases.items():
        r, msg = call(s_, t_, n, *other)
        assert r == 0 and words in msg and "[Resize]" in msg, (what, msg)
    assert call(s, t, 0)[0] == 1                                                                       # nothing to resize: 1
    with pytest.raises(AmtError, match="Resizer"):
        rz.run(src, DeviceSurfaces(dst.Y[:2], dst.U[:2], dst.V[:2], dw, dh, bits))                    # more frames than dst holds
    with pytest.raises(AmtError, match="made for"):
        rz.run(dst, dst)
    k = C.c_int()
    assert ctx.lib.amtgpu_resize_get_program(rz.h, 2, 0, C.byref(k), None, None) == 0 and ctx.lib.amtgpu_resize_get_program(rz.h, 0, 2, C.byref(k), None, None) == 0
    assert ctx.lib.amtgpu_resize_get_program(rz.h, 1, 1, C.byref(k), None, None) == 1 and k.value == R.program(18, 12)[0]
    torch.cuda.synchronize()
    for g, a in zip(download(dst_host, dst_flat), dst_host.flat):
        assert np.array_equal(g, a)                                                                    # still the sentinel, everywhere
    for g, a in zip(download(src_host, src_flat), src_host.flat):
        assert np.array_equal(g, a)
    # ... and the same object and buffers do the work once nothing is wrong: the first two frames
    assert call(s, t, 2)[0] == 1
    torch.cuda.synchronize()
    check_against("two frames", dst_host, download(dst_host, dst_flat), tuple(w[:2] for w in want))
    rz.close()
    rz10.close()
