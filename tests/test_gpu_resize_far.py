"""The resize on frames 2^31 + 5 MiB apart: the three 352 x 240 frames of tests/far_stride_clips.py in its layout L31 to 234 x 160, source
and destination one behind the other in one allocation (the call refuses batches whose byte ranges touch).  The destination frames are
the top left 234 x 160 (117 x 80) containers of that helper's second batch of slots, at its pitch of 352 (176).  Expected bytes come
from the CPU (tests/resize_ref.py); a kernel that forms a frame offset in 32 bits reads or writes one of the helper's decoy windows
instead: wrong bytes, never a fault.  The rest of the destination's windows, its decoy windows and a 4 KiB band around its frames must
stay as they were."""
import numpy as np
import pytest

import far_stride_clips as F
import resize_ref as R
from test_gpu_far_strides import Far, dt_of, planar_clip, planar_extents, planar_frames

pytestmark = pytest.mark.gpu

LAYOUT, DW, DH = "L31", 234, 160


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
    from amatsukaze_amd import DeviceSurfaces, Resizer
    far, bits = env["far"], F.BITS[kind]
    true = F.pictures()[kind]["true"]
    planes = tuple(true[k] for k in "YUV")
    want = R.resize_clip(planes, DW, DH, bits)
    assert all(len(np.unique(w)) > 16 for w in want)
    dslots = ["rd" + k for k in "YUV"]
    far.fill_destination(dslots, [np.zeros_like(p) for p in planes], dt_of(bits))
    watched = far.watch(LAYOUT, planar_extents(kind, dslots))
    src, whole = planar_clip(env, kind, LAYOUT), planar_clip(env, kind, LAYOUT, dslots)
    dst = DeviceSurfaces(whole.Y[:, :DH, :DW], whole.U[:, :DH // 2, :DW // 2], whole.V[:, :DH // 2, :DW // 2], DW, DH, bits)
    assert src.Y.stride(0) * src.Y.element_size() == (1 << 31) + 5 * F.MiB == dst.Y.stride(0) * dst.Y.element_size()
    rz = Resizer(env["ctx"], (F.W, F.H), (DW, DH), bits)
    assert rz.run(src, dst) == F.N
    rz.close()
    env["torch"].cuda.synchronize()
    for k, (g, w) in enumerate(zip(planar_frames(env, kind, LAYOUT, dslots), want)):
        e = np.zeros_like(g)
        e[:, :w.shape[1], :w.shape[2]] = w
        assert np.array_equal(g, e), (kind, "plane", k, "first frame that differs", int(np.argmax([(g[n] != e[n]).any() for n in range(len(g))])))
    far.assert_unchanged(watched)
