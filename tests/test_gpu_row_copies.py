"""ingest_rows_kernel (amtgpu_frames_upload_strided, amtgpu_frames_upload_gather, amtgpu_download_strided) at every lane width the
launcher selects -- 16, 4 and 1 bytes, from the OR of both addresses, both strides and the chunk -- in more than one pass of its grid,
and across two slots of the staging ring.  The device images are flat buffers with guard rows in front and behind and a sentinel in
the padding (tests/copy_cases.py, judged by tests/test_copy_cases_host.py); whole buffers are compared, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import copy_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from amatsukaze_amd import Context
    ctx = Context(0)
    return dict(torch=torch, ctx=ctx, lib=ctx.lib, dev=torch.device("cuda:0"))


@pytest.fixture(scope="module", params=["default-threads", "1-thread"])
def ring(request, env):
    """the context at its default number of staging threads, and another that stages on the calling thread alone"""
    if request.param == "default-threads":
        return env
    from amatsukaze_amd import Context
    ctx = Context(0)
    ctx.check(ctx.lib.amtgpu_context_set_upload_threads(ctx.h, 1))
    return dict(env, ctx=ctx, lib=ctx.lib)


def device_image(e, im, host=None):
    """the image's flat buffer on the device (blank, or `host`), the fill complete: uploads run on a side stream that is not ordered
    behind torch's"""
    d = e["torch"].from_numpy(im.blank() if host is None else host).to(e["dev"])
    assert d.data_ptr() % 16 == 0
    e["torch"].cuda.synchronize()
    return d


def assert_image(e, d, want, what):
    e["ctx"].check(e["lib"].amtgpu_frames_upload_wait(e["ctx"].h))
    e["ctx"].synchronize()
    diff = K.first_difference(d.cpu().numpy(), want)
    assert not diff, f"{what}: {diff}"


def host_rows(rows, stride, lead):
    """rows (n, chunk) laid `stride` apart in pageable memory, `lead` bytes into their allocation -> (allocation, address of row 0)"""
    n, chunk = rows.shape
    buf = np.full(lead + n * stride, 0x3C, np.uint8)
    np.lib.stride_tricks.as_strided(buf[lead:], (n, chunk), (stride, 1))[...] = rows
    return buf, buf.ctypes.data + lead


def strided_upload(e, c, seed):
    im = K.image(c.chunk, c.pitch, c.off, c.nchunks)
    rows = K.random_rows(seed, c.nchunks, c.chunk)
    keep, src = host_rows(rows, c.chunk + 7, 3)
    d = device_image(e, im)
    ctx, lib = e["ctx"], e["lib"]
    ctx.check(lib.amtgpu_frames_upload_strided(ctx.h, d.data_ptr() + im.base, c.pitch, src, c.chunk + 7, c.chunk, c.nchunks))
    assert_image(e, d, im.holding(rows), c.id)


@pytest.mark.parametrize("c", K.STRIDED_UPLOADS, ids=lambda c: c.id)
def test_strided_upload_at_every_lane_width(ring, c):
    strided_upload(ring, c, 11)


def test_strided_upload_across_two_ring_slots(ring):
    """the second slot's rows land behind the first slot's: the destination of its launch starts 6 chunks in"""
    strided_upload(ring, K.TWO_SLOT_STRIDED, 12)


def gather_upload(e, c, nsrc, seed):
    per = c.nchunks // nsrc
    im = K.image(c.chunk, c.pitch, c.off, c.nchunks)
    rows = K.random_rows(seed, c.nchunks, c.chunk)
    stride = c.chunk + 5
    held = [host_rows(rows[i * per:(i + 1) * per], stride, 1 + 2 * i) for i in range(nsrc)]        # odd addresses, each its own
    ptrs = (C.c_void_p * nsrc)(*[p for _, p in held])
    d = device_image(e, im)
    ctx, lib = e["ctx"], e["lib"]
    ctx.check(lib.amtgpu_frames_upload_gather(ctx.h, d.data_ptr() + im.base, c.pitch, ptrs, stride, c.chunk, per, nsrc))
    assert_image(e, d, im.holding(rows), c.id)


@pytest.mark.parametrize("c", K.SMALL_GATHERS, ids=lambda c: c.id)
def test_gather_from_separate_sources_at_odd_addresses(ring, c):
    gather_upload(ring, c, 5, 13)


def test_gather_across_two_ring_slots(ring):
    """the slot boundary falls inside the third source: chunks 0, 1 of it leave with the first slot, 2, 3 with the second"""
    gather_upload(ring, K.TWO_SLOT_GATHER, K.GATHER_SOURCES, 14)


def test_registered_pool_at_every_source_alignment(env):
    """a registered range is read by the kernel where it lies, so the source's offset and stride select the lanes"""
    ctx, lib = env["ctx"], env["lib"]
    c = K.POOL_CASE
    im = K.image(c.chunk, c.pitch, c.off, c.nchunks)
    raw = np.random.default_rng(15).integers(0, 256, 16 + 8 + c.nchunks * 2049, dtype=np.uint8)
    pool = raw[-raw.ctypes.data % 16:]                                        # the offsets below count from a 16-byte boundary
    assert pool.ctypes.data % 16 == 0
    ctx.check(lib.amtgpu_frames_register(ctx.h, C.c_void_p(pool.ctypes.data), pool.size))
    try:
        for (off, stride), lanes in K.POOL_SOURCES.items():
            rows = np.lib.stride_tricks.as_strided(pool[off:], (c.nchunks, c.chunk), (stride, 1))
            d = device_image(env, im)
            ctx.check(lib.amtgpu_frames_upload_strided(ctx.h, d.data_ptr() + im.base, c.pitch, pool.ctypes.data + off, stride, c.chunk,
                                                       c.nchunks))
            assert_image(env, d, im.holding(rows), f"pool + {off}, stride {stride} ({lanes}-byte lanes)")
    finally:
        ctx.check(lib.amtgpu_frames_unregister(ctx.h, C.c_void_p(pool.ctypes.data)))


@pytest.mark.parametrize("c", K.DOWNLOADS, ids=lambda c: c.id)
def test_download_strided_at_every_lane_width(env, c):
    """a small call, a larger one (the pinned landing buffer regrows), the small one again; the host image's padding and guard rows
    survive.  A context of its own: how large the landing buffer is depends on what the context downloaded before."""
    from amatsukaze_amd import Context
    ctx = Context(0)
    e = dict(env, ctx=ctx, lib=ctx.lib)
    big = 3000
    src_im = K.image(c.chunk, c.pitch, c.off, big)
    rows = K.random_rows(16, big, c.chunk)
    d = device_image(e, src_im, src_im.holding(rows))
    for n in (5, big, 5):
        dst_im = K.image(c.chunk, c.chunk + 29, 3, n)
        host = dst_im.blank()
        ctx.check(ctx.lib.amtgpu_download_strided(ctx.h, host.ctypes.data + dst_im.base, dst_im.pitch, d.data_ptr() + src_im.base, c.pitch,
                                                  c.chunk, n))
        diff = K.first_difference(host, dst_im.holding(rows[:n]))
        assert not diff, f"{c.id}, {n} chunks: {diff}"
    assert not K.first_difference(d.cpu().numpy(), src_im.holding(rows))     # the device image is as it was
    ctx.close()
