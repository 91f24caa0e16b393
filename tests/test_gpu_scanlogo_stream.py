"""The streamed ScanLogo session (amtgpu_scanlogo_stream_*, scan_keep_kernel) on the HIP path: whatever the batches look like -- ragged,
one frame at a time, rectangle-only, at awkward addresses, more frames than the store starts with -- the .lgd is byte for byte the CPU
oracle's ScanLogo over the same numpy planes."""
import ctypes as C

import numpy as np
import pytest

import amt_synth as S
from amtlib import Oracle, _ptr

pytestmark = pytest.mark.gpu

# the clip of test_gpu_parity.test_scanlogo_pipeline_lgd_identical
W, H, LW, LH, X, Y0 = 352, 240, 96, 48, 224, 18
SEED, THY, QUOTA, SID = 0x5EED0004, 12, 25, 1041


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return dict(torch=torch, ctx=Context(0), dev=torch.device("cuda:0"))


@pytest.fixture(scope="module")
def orc():
    return Oracle()


_logo = S.make_logo(LW, LH)
_clips = {}


def synth(n=60, x=X):
    """the generator's clip with its logo (and the flat-bordered frames' ring) at (x, Y0); made once, never written to"""
    if (n, x) not in _clips:
        _, alpha, alphaUV = _logo
        c = S.make_clip_np(n, W, H, SEED, alpha, alphaUV, x, Y0, period=20, fade=4, flat_every=2)
        for a in c.values():
            a.setflags(write=False)
        _clips[(n, x)] = c
    return _clips[(n, x)]


def padded(clip, padY, padUV):
    """the same frames in rows padY / padUV bytes longer; the padding is 0xA5, nothing may read it"""
    out = {}
    for k, pad in (("Y", padY), ("U", padUV), ("V", padUV)):
        a = clip[k]
        p = np.full(a.shape[:2] + (a.shape[2] + pad,), 0xA5, np.uint8)
        p[:, :, :a.shape[2]] = a
        out[k] = p
    return out


def oracle_lgd(orc, clip, tmp_path, x=X, quota=QUOTA, name="orc.lgd"):
    """(.lgd bytes, valid frames kept, frames read) of the CPU oracle's ScanLogo over these numpy planes"""
    Y, U, V = clip["Y"], clip["U"], clip["V"]
    nvalid, nread = C.c_int(), C.c_int()
    lo = orc.lib.orc_scanlogo_mt(_ptr(Y), _ptr(U), _ptr(V), Y.strides[0], U.strides[0], Y.shape[2], U.shape[2], W, H, Y.shape[0], x, Y0, LW, LH,
                                 THY, quota, 1, C.byref(nvalid), None, 1, C.byref(nread))
    assert lo, "the oracle made no logo"
    path = tmp_path / name
    assert orc.lib.orc_logo_save(lo, str(path).encode(), b"No Name", SID) == 1
    orc.lib.orc_logo_free(lo)
    return path.read_bytes(), nvalid.value, nread.value


def valid_frames(orc, clip, x=X):
    """AddFrame's verdict per frame"""
    so = orc.lib.orc_scan_create(LW, LH, 1, 1, THY)
    Y, U, V = clip["Y"], clip["U"], clip["V"]
    v = [orc.lib.orc_scan_add_frame_u8(so, Y[i, Y0:, x:].ctypes.data, U[i, Y0 // 2:, x // 2:].ctypes.data, V[i, Y0 // 2:, x // 2:].ctypes.data,
                                       Y.shape[2], U.shape[2]) for i in range(Y.shape[0])]
    orc.lib.orc_scan_free(so)
    return v


def device_clip(gpu, clip, offset=0):
    """the planes in HBM; offset: every plane starts that many bytes into its own allocation"""
    from amatsukaze_amd import DeviceClip
    torch = gpu["torch"]
    planes = []
    for k in "YUV":
        a = clip[k]
        flat = torch.empty(a.size + offset, dtype=torch.uint8, device=gpu["dev"])
        t = flat[offset:].view(a.shape)
        t.copy_(torch.from_numpy(np.array(a)))                # (a writable copy: the shared clips are read-only)
        planes.append(t)
    return DeviceClip(*planes, width=W, height=H)


def part(d, a, b):
    from amatsukaze_amd import DeviceClip
    return DeviceClip(d.Y[a:b], d.U[a:b], d.V[a:b], d.width, d.height)


def new_stream(gpu, x=X, quota=QUOTA):
    from amatsukaze_amd import ScanLogoStream
    return ScanLogoStream(gpu["ctx"], W, H, x, Y0, LW, LH, THY, quota)


def last_error(gpu):
    return gpu["ctx"].lib.amtgpu_last_error(gpu["ctx"].h)


def test_ragged_batches(gpu, orc, tmp_path):
    clip = synth()
    want, nvalid, nread = oracle_lgd(orc, clip, tmp_path)
    assert nvalid == QUOTA
    valid = valid_frames(orc, clip)
    closing = [i for i, v in enumerate(valid) if v][QUOTA - 1]            # the 25th valid frame
    assert nread == closing + 1
    d = device_clip(gpu, clip)
    st = new_stream(gpu)
    f0, before, done_at = 0, 0, None
    sizes = (7, 1, 0, 20, 32)
    assert sum(sizes) == 60 and sum(sizes[:-1]) <= closing                 # the quota fills inside the last batch, not at its end
    for k, n in enumerate(sizes):
        nkept, done = st.feed(part(d, f0, f0 + n))
        f0 += n
        print(f"batch {k}: {n} frames, kept {nkept}, done {done}")
        assert nkept >= before and nkept == min(QUOTA, sum(valid[:f0]))
        before = nkept
        assert done == (closing < f0)
        if done and done_at is None:
            done_at = k
    assert done_at == len(sizes) - 1 and closing < 59
    assert st.status() == {"nread": nread, "nkept": QUOTA, "done": True}
    dst = tmp_path / "ragged.lgd"
    calls = []
    assert st.finish(SID, dst, cb=lambda p, a, b, c: calls.append(p) or 1), last_error(gpu)
    assert dst.read_bytes() == want
    assert calls[-1] == 1.0 and len(calls) > 1 and all(p >= 50.0 for p in calls[:-1])      # driven from 50 % upward, then 1


def test_cut_inside_one_batch(gpu, orc, tmp_path):
    clip = synth()
    want, _, nread = oracle_lgd(orc, clip, tmp_path)
    d = device_clip(gpu, clip)
    st = new_stream(gpu)
    assert st.feed(d) == (QUOTA, True)
    status = st.status()
    assert status == {"nread": nread, "nkept": QUOTA, "done": True} and nread < 60
    assert st.feed(d) == (QUOTA, True) and st.status() == status          # a feed after done: 1, nothing changes
    dst = tmp_path / "one.lgd"
    assert st.finish(SID, dst), last_error(gpu)
    assert dst.read_bytes() == want


def test_rectangle_only_planes_one_frame_per_call(gpu, orc, tmp_path):
    clip = synth()
    want, _, nread = oracle_lgd(orc, clip, tmp_path)
    crop = {"Y": clip["Y"][:, Y0:Y0 + LH, X:X + LW], "U": clip["U"][:, Y0 // 2:(Y0 + LH) // 2, X // 2:(X + LW) // 2],
            "V": clip["V"][:, Y0 // 2:(Y0 + LH) // 2, X // 2:(X + LW) // 2]}
    d = device_clip(gpu, padded(crop, 6, 3))
    Yr, Ur, Vr = d.Y[:, :, :LW], d.U[:, :, :LW // 2], d.V[:, :, :LW // 2]
    assert Yr.stride(1) == LW + 6 and Ur.stride(1) == LW // 2 + 3
    st = new_stream(gpu)
    for i in range(60):
        nkept, done = st.feed_rect(Yr[i:i + 1], Ur[i:i + 1], Vr[i:i + 1])
        assert done == (i + 1 >= nread)
    assert st.status() == {"nread": nread, "nkept": QUOTA, "done": True}
    dst = tmp_path / "rect.lgd"
    assert st.finish(SID, dst), last_error(gpu)
    assert dst.read_bytes() == want


# every width scan_keep_kernel moves a lane's bytes with, per plane kind: (x of the rectangle, row padding Y / UV, byte offset of every
# plane's base).  (224, 0, 0, 0) -- 16 bytes in both -- is what every other test here runs
@pytest.mark.parametrize("x,padY,padUV,offset", [
    (224, 3, 3, 1),       # pitch W + 3 and W/2 + 3, bases one byte into their allocations: single bytes
    (224, 4, 4, 0),       # pitches that are multiples of 4 only: 4-byte vectors in both
    (228, 0, 0, 0),       # luma origin a multiple of 4 only, chroma origin 114: 4 bytes in luma rows, single bytes in chroma rows
    (226, 0, 0, 0),       # chroma origin at an odd sample (113)
])
def test_awkward_addresses(gpu, orc, tmp_path, x, padY, padUV, offset):
    clip = padded(synth(60, x), padY, padUV) if padY or padUV else synth(60, x)
    want, nvalid, nread = oracle_lgd(orc, clip, tmp_path, x=x)           # the oracle reads the same padded arrays
    assert nvalid == QUOTA
    d = device_clip(gpu, clip, offset)
    assert d.pitchY == W + padY and d.pitchUV == W // 2 + padUV and d.Y.data_ptr() % 16 == offset
    st = new_stream(gpu, x=x)
    assert st.feed(part(d, 0, 33))[1] is False
    assert st.feed(part(d, 33, 60)) == (QUOTA, True)
    assert st.status()["nread"] == nread
    dst = tmp_path / "awkward.lgd"
    assert st.finish(SID, dst), last_error(gpu)
    assert dst.read_bytes() == want


def test_store_grows_past_its_first_256_frames(gpu, orc, tmp_path):
    n, nomax = 640, 1 << 30
    clip = synth(n)
    want, nvalid, nread = oracle_lgd(orc, clip, tmp_path, quota=nomax)
    print("oracle keeps", nvalid, "of", n)
    assert nvalid > 256 and nread == n
    st = new_stream(gpu, quota=nomax)          # (a store sized by numMaxFrames would be 7 TB)
    nkept = 0
    for f0 in range(0, n, 64):
        nkept, done = st.feed(device_clip(gpu, {k: clip[k][f0:f0 + 64] for k in "YUV"}))
        assert not done
    assert nkept == nvalid and st.status() == {"nread": n, "nkept": nvalid, "done": False}
    dst = tmp_path / "grown.lgd"
    assert st.finish(SID, dst), last_error(gpu)
    assert dst.read_bytes() == want


def test_errors(gpu, tmp_path):
    from amatsukaze_amd import binding
    lib, ctx = gpu["ctx"].lib, gpu["ctx"]
    d = device_clip(gpu, synth())
    yes, no = binding.CB(lambda *a: 1), binding.CB(lambda *a: 0)
    args = (C.c_void_p(d.Y.data_ptr()), C.c_void_p(d.U.data_ptr()), C.c_void_p(d.V.data_ptr()), d.strideY, d.strideUV, d.pitchY, d.pitchUV)
    dst = tmp_path / "never.lgd"
    # nothing fed
    h = lib.amtgpu_scanlogo_stream_create(ctx.h, W, H, X, Y0, LW, LH, THY, QUOTA)
    assert h
    assert lib.amtgpu_scanlogo_stream_feed(h, *args, 0, None, None) == 1                  # no frames: a no-op
    assert lib.amtgpu_scanlogo_stream_finish(h, SID, str(dst).encode(), yes) == 0
    assert b"Insufficient logo frames" in last_error(gpu)
    # spent: feed and finish refuse, with a message
    nk, dn = C.c_int(-1), C.c_int(-1)
    assert lib.amtgpu_scanlogo_stream_feed(h, *args, 60, C.byref(nk), C.byref(dn)) == 0 and b"finished" in last_error(gpu)
    assert (nk.value, dn.value) == (-1, -1)
    assert lib.amtgpu_scanlogo_stream_feed_rect(h, *args, 1, None, None) == 0 and b"finished" in last_error(gpu)
    assert lib.amtgpu_scanlogo_stream_finish(h, SID, str(dst).encode(), yes) == 0 and b"finished" in last_error(gpu)
    lib.amtgpu_scanlogo_stream_destroy(h)
    # cancel
    h = lib.amtgpu_scanlogo_stream_create(ctx.h, W, H, X, Y0, LW, LH, THY, QUOTA)
    assert lib.amtgpu_scanlogo_stream_feed(h, *args, 60, C.byref(nk), C.byref(dn)) == 1 and (nk.value, dn.value) == (QUOTA, 1)
    assert lib.amtgpu_scanlogo_stream_finish(h, SID, str(dst).encode(), no) == 0
    assert b"Cancel requested" in last_error(gpu)
    assert lib.amtgpu_scanlogo_stream_finish(h, SID, str(dst).encode(), yes) == 0          # spent after a failed finish too
    lib.amtgpu_scanlogo_stream_destroy(h)
    assert not dst.exists()
    # refused rectangles
    for rect, msg in (((W - LW + 2, Y0, LW, LH), b"outside the frame"), ((X, H - LH + 2, LW, LH), b"outside the frame"),
                      ((-2, Y0, LW, LH), b"outside the frame"), ((X, Y0, LW - 1, LH), b"even-sized"), ((X, Y0, LW, 0), b"even-sized")):
        assert not lib.amtgpu_scanlogo_stream_create(ctx.h, W, H, *rect, THY, QUOTA), rect
        assert msg in last_error(gpu), (rect, last_error(gpu))
    # numMaxFrames < 0 counts as 0: closed from the start, nothing read
    h = lib.amtgpu_scanlogo_stream_create(ctx.h, W, H, X, Y0, LW, LH, THY, -5)
    nr = C.c_int64(-1)
    assert lib.amtgpu_scanlogo_stream_feed(h, *args, 60, C.byref(nk), C.byref(dn)) == 1 and (nk.value, dn.value) == (0, 1)
    assert lib.amtgpu_scanlogo_stream_status(h, C.byref(nr), None, None) == 1 and nr.value == 0
    lib.amtgpu_scanlogo_stream_destroy(h)
    ctx.synchronize()


def test_file_entry_points_refuse_a_null_source_path(gpu, tmp_path):
    """both raw-clip entry points read through one reader, which refuses a missing path in its own words before it opens anything"""
    from amatsukaze_amd import binding
    lib, ctx, yes = gpu["ctx"].lib, gpu["ctx"], binding.CB(lambda *a: 1)
    dst = tmp_path / "never.lgd"
    assert lib.amtgpu_scanlogo_file(ctx.h, None, SID, None, str(dst).encode(), X, Y0, LW, LH, THY, QUOTA, yes) == 0
    assert last_error(gpu) == b"null source path"
    assert lib.amtgpu_scanlogo_file_auto(ctx.h, None, SID, None, str(dst).encode(), THY, QUOTA, yes, None, None) == 0
    assert last_error(gpu) == b"null source path"
    assert not dst.exists()


def test_streamed_auto_equals_resident_auto(gpu, tmp_path):
    """the clip of test_gpu_logofind.py, detection and session both fed in batches of 50"""
    from amatsukaze_amd import DeviceClip, ScanLogoAuto, ScanLogoAutoStream
    w, h, lw, lh, x, y0, n = 640, 360, 128, 64, 480, 32, 240
    _, alpha, alphaUV = S.make_logo(lw, lh)
    clip = S.make_clip_np(n, w, h, 0x5EED00A1, alpha, alphaUV, x, y0, period=60, fade=6, flat_every=4)
    torch = gpu["torch"]
    d = DeviceClip(*(torch.from_numpy(clip[k]).to(gpu["dev"]) for k in "YUV"), width=w, height=h)
    resident = tmp_path / "resident.lgd"
    ok, want = ScanLogoAuto(gpu["ctx"], d, SID, resident, THY, QUOTA)
    assert ok, last_error(gpu)
    served = []

    def batches():
        for f0 in range(0, n, 50):
            served.append(f0)
            yield DeviceClip(d.Y[f0:f0 + 50], d.U[f0:f0 + 50], d.V[f0:f0 + 50], w, h)

    streamed = tmp_path / "streamed.lgd"
    got = ScanLogoAutoStream(gpu["ctx"], batches, w, h, SID, streamed, THY, QUOTA)
    assert (got.imgx, got.imgy, got.w, got.h) == (want.imgx, want.imgy, want.w, want.h)
    assert streamed.read_bytes() == resident.read_bytes()
    assert served[:5] == [0, 50, 100, 150, 200] and len(served) < 10      # pass 2 stopped once the quota was full
