"""The temporal noise reduction on decoder surfaces whose frames lie more than 2 GiB apart (amtgpu_temporal_nr_surfaces; layout L31 of
tests/far_stride_clips.py): the three NV12 / P010 pictures in the kind's own slot, the destination in a second far batch behind them
(the call refuses batches whose byte ranges touch, as the cadence renderer does).  Expected values come from the CPU
(tests/temporal_nr_surfaces_ref.py); a kernel that forms a frame offset in 32 bits reads or writes a decoy window instead: wrong bytes,
never a fault.  The decoy windows of the destination and a 4 KiB band around every destination frame stay as they were."""
import numpy as np
import pytest

import far_stride_clips as F
import temporal_nr_surfaces_ref as TS
from test_gpu_far_strides import Far, assert_planes, surface_frames, surfaces

pytestmark = pytest.mark.gpu

D, THRESHOLD, LAYOUT, DST = 1, 3, "L31", "rdS"


@pytest.fixture(scope="module")
def env():
    import torch
    from amatsukaze_amd import Context
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dev = torch.device("cuda:0")
    ctx = Context(0)
    far = Far(torch, dev)
    if far.buf is not None:
        for kind in ("nv12", "p010"):
            far.fill(kind)
        torch.cuda.synchronize()
    e = dict(torch=torch, dev=dev, ctx=ctx, far=far)
    yield e
    ctx.synchronize()
    far.buf16 = far.buf = None
    e.clear()
    ctx.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind", ["nv12", "p010"])
def test_temporal_nr_surfaces_on_far_frames(env, kind):
    from amatsukaze_amd import temporal_nr
    far, bits, msb = env["far"], F.BITS[kind], kind == "p010"
    dt = np.uint8 if bits <= 8 else np.uint16
    true = F.pictures()[kind]["true"]
    planes = (true["Y"], true["U"])
    # the conditions on the pictures, on the CPU, before the GPU result is looked at
    if msb:
        assert all(np.all(p & 63) for p in planes)                                   # every P010 container has non-zero low bits
    want, count = TS.filter_surfaces(planes, D, THRESHOLD, bits, True, msb)
    assert 3 in set(np.unique(count)), sorted(np.unique(count))
    s = TS.shift_of(bits, msb)
    for k, (a, b) in enumerate(zip(TS.unpack(want, bits, True, msb), TS.unpack(planes, bits, True, msb))):
        print(kind, "plane", k, "counts", sorted(np.unique(count)), "changed %.1f %%" % (100 * float(np.mean(a != b))))
        assert np.any(a != b), (kind, "plane", k, "does not change")
    zero = np.zeros((F.N, F.H + F.H // 2, F.W), dt)
    far.fill_destination([DST], [zero], dt)
    watched = far.watch(LAYOUT, {DST: zero[0].nbytes})
    src, dst = surfaces(env, kind, LAYOUT), surfaces(env, kind, LAYOUT, slot=DST)
    assert temporal_nr(env["ctx"], src, dst, distance=D, threshold=THRESHOLD) == (0, F.N)
    env["torch"].cuda.synchronize()
    assert_planes(surface_frames(env, kind, LAYOUT, slot=DST), want, kind)
    assert_planes(surface_frames(env, kind, LAYOUT), planes, (kind, "the source"))
    far.assert_unchanged(watched)
