"""The edge level on frames 2^31 + 5 MiB apart: the three 352 x 240 frames of tests/far_stride_clips.py in its layout L31, source and
destination one behind the other in one allocation (the call refuses batches whose byte ranges touch).  Expected bytes come from the CPU
(tests/edgelevel_ref.py); a kernel that forms a frame offset in 32 bits reads or writes one of that helper's decoy windows instead: wrong
bytes, never a fault.  The decoy windows of the destination and a 4 KiB band around its frames must stay as they were."""
import numpy as np
import pytest

import edgelevel_ref as R
import far_stride_clips as F
from test_gpu_far_strides import Far, assert_planes, dt_of, planar_clip, planar_extents, planar_frames

pytestmark = pytest.mark.gpu

STRENGTH, THRESHOLD, REPAIR, LAYOUT = 16, 10, 2, "L31"


@pytest.fixture(scope="module")
def env():
    import torch
    from amatsukaze_amd import Context
    dev = torch.device("cuda:0")
    ctx = Context(0)
    far = Far(torch, dev)
    if far.buf is not None:
        for kind in ("p8", "p10"):
            far.fill(kind)
        torch.cuda.synchronize()
    e = dict(torch=torch, dev=dev, ctx=ctx, far=far)
    yield e
    ctx.synchronize()
    far.buf16 = far.buf = None
    e.clear()
    ctx.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind", ["p8", "p10"])
def test_three_frames_more_than_2_gib_apart(env, kind):
    from amatsukaze_amd import edge_level
    far, bits = env["far"], F.BITS[kind]
    true = F.pictures()[kind]["true"]
    planes = tuple(true[k] for k in "YUV")
    want = R.filter_clip(planes, bits, STRENGTH, THRESHOLD, REPAIR)
    assert all(not np.array_equal(want[0][n], planes[0][n]) for n in range(F.N))                           # every frame's luma changes
    assert all(np.array_equal(want[k], planes[k]) and planes[k].any() for k in (1, 2))                     # chroma is copied, and is not the zeros below
    dslots = ["rd" + k for k in "YUV"]
    far.fill_destination(dslots, [np.zeros_like(w) for w in want], dt_of(bits))
    watched = far.watch(LAYOUT, planar_extents(kind, dslots))
    src, dst = planar_clip(env, kind, LAYOUT), planar_clip(env, kind, LAYOUT, dslots)
    assert src.Y.stride(0) * src.Y.element_size() == (1 << 31) + 5 * F.MiB == dst.Y.stride(0) * dst.Y.element_size()
    assert edge_level(env["ctx"], src, dst, STRENGTH, THRESHOLD, REPAIR) == F.N
    env["torch"].cuda.synchronize()
    assert_planes(planar_frames(env, kind, LAYOUT, dslots), want, kind)
    far.assert_unchanged(watched)
