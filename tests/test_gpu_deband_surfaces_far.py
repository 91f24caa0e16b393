"""The deband on decoder surfaces whose frames lie 2^31 + 5 MiB apart (amtgpu_deband_run_surfaces; layout L31 of
tests/far_stride_clips.py): the three 352 x 240 P010 pictures in the kind's own slot, the destination in a second far batch behind them
(the call refuses batches whose byte ranges touch).  Expected bytes come from the CPU (tests/deband_surfaces_ref.py); a kernel that forms
a frame offset in 32 bits reads or writes one of the helper's decoy windows instead: wrong bytes, never a fault.  The decoy windows of
the destination and a 4 KiB band around its frames must stay as they were."""
import numpy as np
import pytest

import deband_surfaces_ref as DS
import far_stride_clips as F
import temporal_nr_surfaces_ref as TS
from test_gpu_far_strides import Far, assert_planes, surface_frames, surfaces

pytestmark = pytest.mark.gpu

RADIUS, THRESHOLD, SEED, LAYOUT, DST = 25, 32767, 9, "L31", "rdS"


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
    from amatsukaze_amd import Debander
    far, kind, bits = env["far"], "p010", F.BITS["p010"]
    true = F.pictures()[kind]["true"]
    planes = (true["Y"], true["U"])
    assert all(np.all(p & 63) for p in planes)                                       # every P010 container has non-zero low bits
    want = DS.deband_surfaces(planes, bits, True, True, RADIUS, THRESHOLD, 2, True, SEED)
    for n in range(F.N):                                                             # every frame changes, in luma and in chroma
        assert all(not np.array_equal(w[n] >> 6, p[n] >> 6) for w, p in zip(want, planes))
    assert all(not np.any(w & 63) for w in want)
    zero = np.zeros((F.N, F.H + F.H // 2, F.W), np.uint16)
    far.fill_destination([DST], [zero], np.uint16)
    watched = far.watch(LAYOUT, {DST: zero[0].nbytes})
    src, dst = surfaces(env, kind, LAYOUT), surfaces(env, kind, LAYOUT, slot=DST)
    assert src.Y.stride(0) * src.Y.element_size() == (1 << 31) + 5 * F.MiB == dst.U.stride(0) * dst.U.element_size()
    db = Debander(env["ctx"], (F.W, F.H), bits, RADIUS, THRESHOLD, 2, True, SEED)
    assert db.run(src, dst) == F.N
    db.close()
    env["torch"].cuda.synchronize()
    assert_planes(surface_frames(env, kind, LAYOUT, slot=DST), want, kind)
    assert_planes(surface_frames(env, kind, LAYOUT), planes, (kind, "the source"))
    far.assert_unchanged(watched)
    assert TS.shift_of(bits, True) == 6
