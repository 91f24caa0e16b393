"""The resize on decoder surfaces whose frames lie 2^31 + 5 MiB apart (amtgpu_resize_run_surfaces; layout L31 of
tests/far_stride_clips.py): the three 352 x 240 P010 pictures in the kind's own slot to 234 x 160, the destination the top left
234 x 160 (UV rows: 234 containers by 80) of a second far batch behind them, at the slot's pitch of 352 (the call refuses batches whose
byte ranges touch).  Expected bytes come from the CPU (tests/resize_surfaces_ref.py); a kernel that forms a frame offset in 32 bits
reads or writes one of the helper's decoy windows instead: wrong bytes, never a fault.  The rest of the destination's windows, its
decoy windows and a 4 KiB band around its frames must stay as they were."""
import numpy as np
import pytest

import far_stride_clips as F
import resize_surfaces_ref as RS
from test_gpu_far_strides import Far, assert_planes, surface_frames, surfaces

pytestmark = pytest.mark.gpu

LAYOUT, DST, DW, DH = "L31", "rdS", 234, 160


@pytest.fixture(scope="module")
def env():
    import torch
    from amatsukaze_amd import Context
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dev = torch.device("cuda:0")
    ctx = Context(0)
    far = Far(torch, dev)
    if far.buf is not None:
        far.fill("p010")
        torch.cuda.synchronize()
    e = dict(torch=torch, dev=dev, ctx=ctx, far=far)
    yield e
    ctx.synchronize()
    far.buf16 = far.buf = None
    e.clear()
    ctx.close()
    torch.cuda.empty_cache()


def test_three_p010_frames_more_than_2_gib_apart(env):
    from amatsukaze_amd import DeviceSurfaces, Resizer
    far, kind, bits = env["far"], "p010", F.BITS["p010"]
    true = F.pictures()[kind]["true"]
    planes = (true["Y"], true["U"])
    assert all(np.all(p & 63) for p in planes)                                       # every P010 container has non-zero low bits
    want = RS.resize_surfaces(planes, DW, DH, bits, True, True)
    assert all(len(np.unique(w)) > 16 for w in want) and want[1].shape == (F.N, DH // 2, DW)
    zero = np.zeros((F.N, F.H + F.H // 2, F.W), np.uint16)
    far.fill_destination([DST], [zero], np.uint16)
    watched = far.watch(LAYOUT, {DST: zero[0].nbytes})
    src, whole = surfaces(env, kind, LAYOUT), surfaces(env, kind, LAYOUT, slot=DST)
    dst = DeviceSurfaces(whole.Y[:, :DH, :DW], whole.U[:, :DH // 2, :DW], None, DW, DH, bits, interleaved=True, msb=True)
    assert src.Y.stride(0) * src.Y.element_size() == (1 << 31) + 5 * F.MiB == dst.U.stride(0) * dst.U.element_size()
    rz = Resizer(env["ctx"], (F.W, F.H), (DW, DH), bits)
    assert rz.run(src, dst) == F.N
    rz.close()
    env["torch"].cuda.synchronize()
    expected = []
    for g, w in zip(surface_frames(env, kind, LAYOUT, slot=DST), want):
        e = np.zeros_like(g)
        e[:, :w.shape[1], :w.shape[2]] = w
        expected.append(e)
    assert_planes(surface_frames(env, kind, LAYOUT, slot=DST), expected, kind)
    assert_planes(surface_frames(env, kind, LAYOUT), planes, (kind, "the source"))
    far.assert_unchanged(watched)
