"""The frame metrics straight from decoder surfaces (amtgpu_framestats_surfaces): all three 16-bit kernel forms at MSB alignment, depths 9,
10, 12 and 15, heights around the tile heights, batches that cross the 32-frame run, containers with non-zero (random, and all-ones) low
bits, 0xFFFF in every byte of the allocation that is no sample -- byte-equal to oracle/frame_stats_oracle.py on container >> shift, never
to the library itself.  LSB descriptors (NV12, planar 10-bit) take the plain kernels; the weave route gives the same records; bad
descriptors are refused with a message.  tests/test_surface_stats_abi.py shows that these inputs would catch a wrong shift."""
import ctypes as C

import numpy as np
import pytest

import plane_edge_clips as P
import surface_clips as SC
import surface_stats_clips as S
from plane_edge_clips import FS

pytestmark = pytest.mark.gpu

WORDS = ("DIFF_TOP", "DIFF_BOT", "VERT", "COMB", "COMB_PREV", "SUM", "VERT_PREV", "reserved")
SENTINEL = -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return dict(torch=torch, ctx=Context(0), dev=torch.device("cuda:0"))


def assert_records(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        n, k = bad[0]
        raise AssertionError(f"{what}: {len(bad)} words differ, first frame {n} {WORDS[k]}: got {got[n, k]}, want {want[n, k]}; "
                             f"words off: {sorted({WORDS[j] for j in bad[:, 1]})}")


def luma_surfaces(t, W, H, bits, msb):
    """the Y planes of t (N, H, pitch) as a P010-like descriptor without chroma: the metrics never look at it"""
    from amatsukaze_amd import DeviceSurfaces
    return DeviceSurfaces(t, None, None, W, H, bits, interleaved=True, msb=msb)


def surface_metrics(gpu, fs, surf, prev=None):
    """(N, 8) records; one more row of the output holds a sentinel and must keep it"""
    torch = gpu["torch"]
    n = surf.num_frames
    out = torch.full((n + 1, 8), SENTINEL, dtype=torch.int64, device=gpu["dev"])
    fs.run_device_surfaces(surf, out, prev)
    gpu["ctx"].synchronize()
    h = out.cpu().numpy()
    assert np.all(h[n] == SENTINEL), "words beyond nframes * 8 were written"
    return h[:n].astype(np.uint64)


def test_case_list_reaches_every_form():
    for f, (W, pitch) in S.FORMS.items():
        assert P.predicted_form("frame_stats", W, pitch, 2) == f
    assert {c[0] for c in S.GEOMETRY_CASES} == {c[0] for c in S.BATCH_CASES} == {c[0] for c in S.LOW_BITS_CASES} == set(S.FORMS)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_msb_surfaces(gpu, case):
    """without a previous picture, with the one in front of the batch in the same allocation, and with one in an allocation of its own"""
    from amatsukaze_amd import FrameStats
    f, bits, H, N, kind = case
    W, pitch = S.FORMS[f]
    clip, sep = S.clip_of(case)
    t = P.to_device(gpu["torch"], gpu["dev"], clip)
    tsep = P.to_device(gpu["torch"], gpu["dev"], sep)
    assert t.shape == (N + 1, H, pitch) and t.stride(0) == (H + 2) * pitch
    fs = FrameStats(gpu["ctx"], W, H, bits)
    batch = luma_surfaces(t[1:], W, H, bits, True)
    runs = S.runs_of(case)
    prevs = (None, luma_surfaces(t[0:1], W, H, bits, True), luma_surfaces(tsep, W, H, bits, True))
    for (b, p), dprev, what in zip(runs, prevs, ("no previous picture", "previous picture in the allocation", "previous picture apart")):
        assert_records(surface_metrics(gpu, fs, batch, dprev), S.truth(b, p, bits), f"{S.case_id(case)} {what}")


def lsb_case(gpu, bits, W, pitch, H, N):
    from amatsukaze_amd import FrameStats
    rng = np.random.default_rng([bits, W, pitch, H, N])
    Y = rng.integers(0, 1 << bits, (N + 1, H, W)).astype(P.dtype_of(bits))
    clip = P.embed(Y, pitch, rows_after=2)
    t = P.to_device(gpu["torch"], gpu["dev"], clip)
    fs = FrameStats(gpu["ctx"], W, H, bits)
    for prev, dprev, tprev in ((None, None, None), (clip.sub(0, 1), luma_surfaces(t[0:1], W, H, bits, False), t[0])):
        want = P.true_metrics(clip.sub(1), prev)
        got = surface_metrics(gpu, fs, luma_surfaces(t[1:], W, H, bits, False), dprev)
        assert_records(got, want, f"{bits}-bit LSB surfaces")
        plain = gpu["torch"].full((N, 8), SENTINEL, dtype=gpu["torch"].int64, device=gpu["dev"])
        fs.run_device(t[1:], plain, prevY=tprev)
        gpu["ctx"].synchronize()
        assert_records(got, plain.cpu().numpy().astype(np.uint64), f"{bits}-bit LSB surfaces against run_device")


def test_nv12_surfaces_with_a_padded_pitch(gpu):
    lsb_case(gpu, 8, 45, 64, 29, 3)


def test_planar_lsb_10_bit_surfaces(gpu):
    lsb_case(gpu, 10, 37, 48, 21, 3)


def test_p010_route_equality(gpu):
    """run_surfaces on P010 pictures = weave_fields(msb=True) of the whole pictures followed by run = the oracle"""
    from amatsukaze_amd import DeviceClip, DeviceSurfaces, FrameStats, weave_fields
    torch, dev = gpu["torch"], gpu["dev"]
    W, H, N, bits = 48, 24, 5, 10
    rng = np.random.default_rng(4810)
    clip = {"Y": rng.integers(0, 1 << bits, (N, H, W)).astype(np.uint16), "U": rng.integers(0, 1 << bits, (N, H // 2, W // 2)).astype(np.uint16),
            "V": rng.integers(0, 1 << bits, (N, H // 2, W // 2)).astype(np.uint16)}
    surf = SC.to_surfaces(clip, bits, True, True, rng, padY=8, padUV=8, fill=0xFFFF)
    assert np.array_equal(SC.from_surfaces(surf, W, H, bits, True, True)["Y"], clip["Y"])
    dY, dUV = (torch.from_numpy(surf[k].view(np.int16)).to(dev) for k in ("Y", "U"))
    fs = FrameStats(gpu["ctx"], W, H, bits)
    direct = fs.run_surfaces(DeviceSurfaces(dY, dUV, None, W, H, bits, interleaved=True, msb=True))
    planar = DeviceClip(*(torch.zeros(s, dtype=torch.int16, device=dev) for s in ((N, H, W), (N, H // 2, W // 2), (N, H // 2, W // 2))),
                        width=W, height=H, bits=bits)
    weave_fields(gpu["ctx"], dY, dUV, None, planar, nv12=True, msb=True)
    woven = fs.run(planar)
    assert_records(direct, FS.frame_metrics(clip["Y"]), "P010 surfaces against the oracle")
    assert_records(direct, woven, "P010 surfaces against the weave route")


def test_refusals(gpu):
    from amatsukaze_amd import AmtError, FrameStats
    torch, dev, ctx = gpu["torch"], gpu["dev"], gpu["ctx"]
    W, H, N = 37, 21, 2
    t16 = torch.full((N + 1, H, 48), 0x1234, dtype=torch.int16, device=dev)
    t16w = torch.full((1, H, 56), 0x1234, dtype=torch.int16, device=dev)
    t8 = torch.full((N, H, 48), 0x12, dtype=torch.uint8, device=dev)
    out = torch.full((N + 1, 8), SENTINEL, dtype=torch.int64, device=dev)
    fs10, fs8 = FrameStats(ctx, W, H, 10), FrameStats(ctx, W, H, 8)
    batch = luma_surfaces(t16[1:], W, H, 10, True)
    with pytest.raises(AmtError, match="another depth"):
        fs10.run_device_surfaces(luma_surfaces(t16[1:], W, H, 12, True), out)
    with pytest.raises(AmtError, match="MSB-aligned surfaces are 16-bit containers"):
        fs8.run_device_surfaces(luma_surfaces(t8, W, H, 8, True), out)
    with pytest.raises(AmtError, match="previous picture must have the batch's"):
        fs10.run_device_surfaces(batch, out, luma_surfaces(t16w, W, H, 10, True))
    with pytest.raises(AmtError, match="previous picture must have the batch's"):
        fs10.run_device_surfaces(batch, out, luma_surfaces(t16[0:1], W, H, 10, False))
    with pytest.raises(AmtError, match="previous picture must have the batch's"):
        fs10.run_device_surfaces(batch, out, luma_surfaces(t16[0:1], W, H, 12, True))
    with pytest.raises(AmtError, match="unsupported frame format"):
        FrameStats(ctx, W, H, 16)
    # negative nframes: 0 with a message; nframes == 0: 1, nothing written, even with no descriptor to read
    d = batch.ref()
    assert ctx.lib.amtgpu_framestats_surfaces(fs10.h, C.byref(d), None, -1, C.c_void_p(out.data_ptr())) == 0
    assert b"negative frame count" in ctx.lib.amtgpu_last_error(ctx.h)
    assert ctx.lib.amtgpu_framestats_surfaces(fs10.h, C.byref(d), None, 0, C.c_void_p(out.data_ptr())) == 1
    assert ctx.lib.amtgpu_framestats_surfaces(fs10.h, None, None, 0, None) == 1
    fs10.run_device_surfaces(luma_surfaces(t16[:0], W, H, 10, True), out)
    ctx.synchronize()
    assert bool((out == SENTINEL).all()), "a refused or empty call wrote records"
    # the object still works
    got = surface_metrics(gpu, fs10, batch)
    assert_records(got, FS.frame_metrics(np.full((N, H, W), 0x1234 >> 6, np.uint16)), "after the refusals")
