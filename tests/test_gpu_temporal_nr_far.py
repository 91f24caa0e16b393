"""The temporal noise reduction on frames 2^31 + 5 MiB apart: the three 352 x 240 frames of tests/far_stride_clips.py in its layout L31,
source and destination one behind the other in one allocation (the call refuses batches whose byte ranges touch, like the cadence
renderer), temporal_distance 1 so that every output frame reads every far frame.  Expected bytes come from the CPU
(tests/temporal_nr_ref.py); a kernel that forms a frame offset in 32 bits reads or writes one of that helper's decoy windows instead:
wrong bytes, never a fault.  The decoy windows of the destination and a 4 KiB band around its frames must stay as they were."""
import numpy as np
import pytest

import far_stride_clips as F
import temporal_nr_ref as R
from test_gpu_far_strides import Far, assert_planes, dt_of, planar_clip, planar_extents, planar_frames

pytestmark = pytest.mark.gpu

DISTANCE, THRESHOLD, LAYOUT = 1, 3, "L31"


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
    from amatsukaze_amd import temporal_nr
    far, bits = env["far"], F.BITS[kind]
    true = F.pictures()[kind]["true"]
    planes = tuple(true[k] for k in "YUV")
    want = R.filter_clip(planes, DISTANCE, THRESHOLD, bits)
    assert int(want[3].max()) == 3 and all(not np.array_equal(want[k], planes[k]) for k in range(3))        # frames pass, samples change
    dslots = ["rd" + k for k in "YUV"]
    far.fill_destination(dslots, [np.zeros_like(w) for w in want[:3]], dt_of(bits))
    watched = far.watch(LAYOUT, planar_extents(kind, dslots))
    src, dst = planar_clip(env, kind, LAYOUT), planar_clip(env, kind, LAYOUT, dslots)
    assert src.Y.stride(0) * src.Y.element_size() == (1 << 31) + 5 * F.MiB
    assert temporal_nr(env["ctx"], src, dst, distance=DISTANCE, threshold=THRESHOLD) == (0, F.N)
    env["torch"].cuda.synchronize()
    assert_planes(planar_frames(env, kind, LAYOUT, dslots), want[:3], kind)
    far.assert_unchanged(watched)
