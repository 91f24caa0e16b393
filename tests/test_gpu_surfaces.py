"""Decoder surfaces (NV12, P010 / P012, planar MSB) on the HIP path: the rectangle extraction against numpy byte for byte on every lane
width, ScanLogo sessions fed with surfaces against the CPU reference's .lgd (tests/scanlogo_ref.py), the logo finder's sums of MSB-aligned
Y planes, the automatic streamed scan over P010 batches, the field weave from MSB pictures against the oracle, and what must be refused.
The surfaces come from tests/surface_clips.py (pinned on the CPU by test_surface_ref_host.py): MSB-aligned containers carry random
non-zero low bits, so a path that forgets the shift fails."""
import ctypes as C

import numpy as np
import pytest

import logofind_ref as LR
import scanlogo_hibit_clips as K
import surface_clips as SC
from amtlib import Oracle, _ptr
from test_ingest import CASES as WEAVE_CASES

pytestmark = pytest.mark.gpu

THY, QUOTA, SID = K.THY, K.QUOTA, K.SID


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return dict(torch=torch, ctx=Context(0), dev=torch.device("cuda:0"))


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def refdir(tmp_path_factory):
    return tmp_path_factory.mktemp("surfaces_ref")


def last_error(gpu):
    return gpu["ctx"].lib.amtgpu_last_error(gpu["ctx"].h)


def to_dev(gpu, a, offset=0):
    """the plane in HBM, starting `offset` bytes into its own allocation; 16-bit containers as int16"""
    torch = gpu["torch"]
    a = np.array(a, order="C")            # (a copy: the shared clips are read-only)
    flat = torch.empty(a.nbytes + offset, dtype=torch.uint8, device=gpu["dev"])
    t = flat[offset:]
    if a.dtype == np.uint16:
        t = t.view(torch.int16)
        a = a.view(np.int16)
    t = t.view(a.shape)
    t.copy_(torch.from_numpy(a))
    return t


def to_host(t, dt):
    return t.cpu().numpy().view(dt)


def device_surfaces(gpu, surf, W, H, bits, interleaved, msb, offset=0):
    from amatsukaze_amd import DeviceSurfaces
    return DeviceSurfaces(to_dev(gpu, surf["Y"], offset), to_dev(gpu, surf["U"], offset), to_dev(gpu, surf["V"], offset) if surf["V"] is not None else None,
                          width=W, height=H, bits=bits, interleaved=bool(interleaved), msb=bool(msb))


def part(d, a, b):
    from amatsukaze_amd import DeviceSurfaces
    return DeviceSurfaces(d.Y[a:b], d.U[a:b], d.V[a:b] if d.V is not None else None, d.width, d.height, d.bits, d.interleaved, d.msb)


def fill_of(bits):
    return 0xA5 if bits == 8 else 0xA5A5


# ---- a. extraction against numpy, byte for byte ----
LAYOUTS = [(8, 1, 0), (10, 1, 1), (10, 0, 1), (10, 1, 0), (12, 1, 1), (12, 0, 1), (12, 1, 0)]          # (bits, interleaved, msb)
_small = {}


def small_clip(bits):
    """5 random frames of 64 x 40, once per depth"""
    if bits not in _small:
        rng = np.random.default_rng(0x5F00 + bits)
        dt = np.uint8 if bits == 8 else np.uint16
        c = {"Y": rng.integers(0, 1 << bits, (5, 40, 64)).astype(dt), "U": rng.integers(0, 1 << bits, (5, 20, 32)).astype(dt),
             "V": rng.integers(0, 1 << bits, (5, 20, 32)).astype(dt)}
        for a in c.values():
            a.setflags(write=False)
        _small[bits] = c
    return _small[bits]


def extract(gpu, d, rect, dpadY=16, dpadUV=8, doffset=0):
    """amtgpu_surfaces_extract_rect into planes whose rows are dpadY / dpadUV samples longer than the rectangle's and pre-filled with a
    sentinel; returns the whole planes (padding included) and the sentinel"""
    torch = gpu["torch"]
    x, y, w, h = rect
    n = d.num_frames
    dt = np.uint8 if d.bits == 8 else np.uint16
    sent = 0x5A if d.bits == 8 else 0x5A5A
    outs = [to_dev(gpu, np.full((n, hh, ww + pad), sent, dt), doffset) for hh, ww, pad in ((h, w, dpadY), (h // 2, w // 2, dpadUV), (h // 2, w // 2, dpadUV))]
    desc = d.ref()
    es = d.es
    ok = gpu["ctx"].lib.amtgpu_surfaces_extract_rect(gpu["ctx"].h, C.byref(desc), x, y, w, h, n, *(C.c_void_p(t.data_ptr()) for t in outs),
                                                      int(outs[0].stride(0)) * es, int(outs[1].stride(0)) * es, int(outs[0].stride(1)),
                                                      int(outs[1].stride(1)))
    assert ok == 1, last_error(gpu)
    torch.cuda.synchronize()
    return [to_host(t, dt) for t in outs], sent


def check_extract(gpu, clip, W, H, bits, interleaved, msb, rect, padY, padUV, offset=0, doffset=0):
    rng = np.random.default_rng(bits * 8 + interleaved * 2 + msb)
    surf = SC.to_surfaces(clip, bits, interleaved, msb, rng, padY, padUV, fill_of(bits))
    d = device_surfaces(gpu, surf, W, H, bits, interleaved, msb, offset)
    got, sent = extract(gpu, d, rect, doffset=doffset)
    want = SC.crop(clip, *rect)
    x, y, w, h = rect
    for k, g, ww in zip("YUV", got, (w, w // 2, w // 2)):
        assert g[:, :, :ww].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (k, rect)
        assert np.all(g[:, :, ww:] == sent), (k, "destination padding written")


# Lane widths (bytes one lane LOADS; luma / chroma), 8-bit NV12 | 16-bit interleaved | 16-bit planar:
#   (8, 8, 48, 24) padded by 16 containers:   4 / 4    | 16 / 16 | 16 / 4  (luma origin 8 B | 16 B; planar chroma origin 4 samples = 8 B)
#   (0, 0, 48, 24), (16, 16, 48, 24) unpadded: 16 / 16 | 16 / 16 | 16 / 16 (the second ends on the surface's last sample: nothing rounds up)
#   (0, 0, 64, 40) whole frame:                16 / 16 | 16 / 16 | 16 / 16
@pytest.mark.parametrize("bits,interleaved,msb", LAYOUTS)
@pytest.mark.parametrize("rect,padY,padUV", [((8, 8, 48, 24), 16, 16), ((0, 0, 48, 24), 0, 0), ((16, 16, 48, 24), 0, 0), ((0, 0, 64, 40), 0, 0)])
def test_extract_small_surface(gpu, bits, interleaved, msb, rect, padY, padUV):
    check_extract(gpu, small_clip(bits), 64, 40, bits, interleaved, msb, rect, padY, padUV)


#   "A" (224, 18, 96, 48) over 352 x 240:      16 / 16 | 16 / 16 | 16 / 16  (every origin, pitch, stride and row a multiple of 16 bytes)
#   "odd" (226, 18, 66, 40): chroma origin 113, wUV 33
#                                               single bytes, chroma as byte pairs (origins 226 B) | 4 / 4 (chroma origin 113 pairs = 452 B)
#                                               | 4 / 2 (chroma origin 226 B)
#   "A" with every plane one sample into its allocation (source and destination): single samples, interleaved chroma pair by pair
@pytest.mark.parametrize("bits,interleaved,msb", LAYOUTS)
@pytest.mark.parametrize("name,offset_samples", [("A", 0), ("odd", 0), ("A", 1)])
def test_extract_logo_rectangles(gpu, bits, interleaved, msb, name, offset_samples):
    W, H, lw, lh, x, y, _ = K.geometry(name)
    clip = {k: K.clip(name, bits)[k][:5] for k in "YUV"}
    off = offset_samples * (1 if bits == 8 else 2)
    check_extract(gpu, clip, W, H, bits, interleaved, msb, (x, y, lw, lh), 0, 0, offset=off, doffset=off)


def test_extract_rect_python_mirror(gpu):
    """extract_rect allocates tight planes of the surfaces' container type"""
    from amatsukaze_amd import extract_rect
    rng = np.random.default_rng(7)
    clip = small_clip(10)
    d = device_surfaces(gpu, SC.to_surfaces(clip, 10, 1, 1, rng, 16, 16, 0xA5A5), 64, 40, 10, 1, 1)
    Y, U, V = extract_rect(gpu["ctx"], d, 8, 8, 48, 24)
    gpu["torch"].cuda.synchronize()
    want = SC.crop(clip, 8, 8, 48, 24)
    assert tuple(Y.shape) == (5, 24, 48) and tuple(U.shape) == tuple(V.shape) == (5, 12, 24)
    for k, t in zip("YUV", (Y, U, V)):
        assert to_host(t, np.uint16).tobytes() == np.ascontiguousarray(want[k]).tobytes(), k


# ---- b. ScanLogo sessions fed with surfaces ----
def new_stream(gpu, name, bits):
    from amatsukaze_amd import ScanLogoStream
    W, H, lw, lh, x, y, _ = K.geometry(name)
    return ScanLogoStream(gpu["ctx"], W, H, x, y, lw, lh, THY, QUOTA, bits=bits)


def finished(gpu, st, path):
    assert st.finish(SID, path), last_error(gpu)
    return path.read_bytes()


@pytest.mark.parametrize("name,bits,interleaved,msb", [("A", 8, 1, 0), ("A", 10, 1, 1), ("A", 12, 0, 1), ("odd", 10, 1, 1)])
def test_session_fed_with_surfaces(gpu, orc, refdir, tmp_path, name, bits, interleaved, msb):
    W, H, _, _, _, _, n = K.geometry(name)
    want, info = K.reference(orc, name, bits, refdir)
    assert want is not None and (info["kept"], info["nread"]) == (25, 43)
    rng = np.random.default_rng(bits + 100)
    d = device_surfaces(gpu, SC.to_surfaces(K.clip(name, bits), bits, interleaved, msb, rng, 0, 0, fill_of(bits)), W, H, bits, interleaved, msb)
    st = new_stream(gpu, name, bits)
    f0, seen = 0, []
    for k in (7, 1, 13, n - 21):                      # ragged batches: the scratch grows twice
        seen.append(st.feed_surfaces(part(d, f0, f0 + k)))
        f0 += k
    assert [s[1] for s in seen] == [False, False, False, True] and seen[-1][0] == QUOTA
    assert all(a[0] <= b[0] for a, b in zip(seen, seen[1:]))
    assert st.status() == {"nread": info["nread"], "nkept": info["kept"], "done": True}
    assert finished(gpu, st, tmp_path / "surfaces.lgd") == want


def test_session_mixes_feed_and_feed_surfaces(gpu, orc, refdir, tmp_path):
    from amatsukaze_amd import DeviceClip
    W, H, lw, lh, x, y, n = K.geometry("A")
    want, info = K.reference(orc, "A", 10, refdir)
    clip = K.clip("A", 10)
    rng = np.random.default_rng(5)
    d = device_surfaces(gpu, SC.to_surfaces(clip, 10, 1, 1, rng, 0, 0, 0xA5A5), W, H, 10, 1, 1)
    planar = DeviceClip(*(to_dev(gpu, clip[k]) for k in "YUV"), width=W, height=H, bits=10)
    crop = SC.crop(clip, x, y, lw, lh)
    st = new_stream(gpu, "A", 10)
    assert st.feed_surfaces(part(d, 0, 9))[1] is False
    assert st.feed(DeviceClip(planar.Y[9:20], planar.U[9:20], planar.V[9:20], W, H, 10))[1] is False
    assert st.feed_rect(*(to_dev(gpu, crop[k][20:24]) for k in "YUV"))[1] is False
    assert st.feed_surfaces(part(d, 24, 31))[1] is False
    # planar LSB surfaces go straight to feed
    lsb = device_surfaces(gpu, SC.to_surfaces({k: clip[k][31:40] for k in "YUV"}, 10, 0, 0, rng, 3, 1, 0xA5A5), W, H, 10, 0, 0)
    assert st.feed_surfaces(lsb)[1] is False
    assert st.feed_surfaces(part(d, 40, n)) == (QUOTA, True)
    assert st.status() == {"nread": info["nread"], "nkept": QUOTA, "done": True}
    assert st.feed_surfaces(d) == (QUOTA, True)                                          # a feed after done changes nothing
    assert finished(gpu, st, tmp_path / "mixed.lgd") == want


# ---- c. logo finder sums ----
@pytest.mark.parametrize("bits", [10, 16])
@pytest.mark.parametrize("pitch", [256, 250])        # buffer-load form | sample-wise form (an unpadded pitch that is no multiple of 4)
def test_finder_sums_of_msb_planes(gpu, bits, pitch):
    """W = 250: two column waves, not a multiple of 4; H = 19: first, interior and last tiles; 5 frames: the two row sets swap"""
    from amatsukaze_amd import DeviceSurfaces, LogoFinder
    W, H, n = 250, 19, 5
    rng = np.random.default_rng(bits * 1000 + pitch)
    lsb = rng.integers(0, 1 << bits, (n, H, W)).astype(np.uint16)
    Y = np.full((n, H, pitch), 0xA5A5, np.uint16)
    Y[:, :, :W] = SC.msb_containers(lsb, bits, rng)
    if bits < 16:
        assert np.all(Y[:, :, :W] & ((1 << (16 - bits)) - 1))
    lf = LogoFinder(gpu["ctx"], W, H, bits)
    lf.add_surfaces(DeviceSurfaces(to_dev(gpu, Y), None, None, W, H, bits, True, True))
    S1, SM = lf.sums()
    assert lf.nframes == n
    want = LR.sums(lsb, W, H)
    assert np.array_equal(np.concatenate([S1.ravel(), SM.ravel()]), want)
    # LSB surfaces forward to add_batch: the same planes again double the sums
    lf.add_surfaces(DeviceSurfaces(to_dev(gpu, lsb), None, None, W, H, bits, True, False))
    S1, SM = lf.sums()
    assert np.array_equal(np.concatenate([S1.ravel(), SM.ravel()]), 2 * want)


# ---- d. automatic streamed scan over P010 batches ----
def test_auto_stream_over_p010_batches(gpu, orc, refdir, tmp_path):
    from amatsukaze_amd import ScanLogoAutoStream
    W, H, _, _, _, _, n = K.geometry("auto")
    want, info = K.reference(orc, "auto", 10, refdir, rect=K.AUTO_RECT)
    assert want is not None
    rng = np.random.default_rng(11)
    d = device_surfaces(gpu, SC.to_surfaces(K.clip("auto", 10), 10, 1, 1, rng, 0, 0, 0xA5A5), W, H, 10, 1, 1)
    served = []

    def batches():
        for f0 in range(0, n, 60):
            served.append(f0)
            yield part(d, f0, f0 + 60)

    dst = tmp_path / "auto_p010.lgd"
    got = ScanLogoAutoStream(gpu["ctx"], batches, W, H, SID, dst, THY, QUOTA, bits=10)
    assert (got.imgx, got.imgy, got.w, got.h) == K.AUTO_RECT
    assert dst.read_bytes() == want
    assert served[:4] == [0, 60, 120, 180] and len(served) < 8          # pass 2 stopped once the quota was full


# ---- e. weave from MSB pictures ----
#   (66, 28, 10, pad 2, NV12): 136-byte rows -- the element path and the 16-bit NV12 split
#   (352, 240, 12, pad 32, planar): every row 16-byte aligned -- the vector path
#   (72, 8, 10, planar, pitches 80 / 40): vector path whose 72-byte chroma rows end in a partial vector
def _weave_cases():
    out = [(W, H, bits, W + pad, (W if nv12 else W // 2) + pad, W + 16, W // 2 + 8, nv12) for W, H, bits, pad, nv12 in WEAVE_CASES if bits > 8]
    assert len(out) == 2
    return out + [(72, 8, 10, 80, 40, 80, 40, False)]


@pytest.mark.parametrize("W,H,bits,spY,spUV,pY,pUV,nv12", _weave_cases())
def test_weave_from_msb_pictures(gpu, orc, W, H, bits, spY, spUV, pY, pUV, nv12):
    from amatsukaze_amd import DeviceClip, weave_fields
    torch = gpu["torch"]
    rng = np.random.default_rng(W * 7 + H + bits)
    P, top, bot = 3, [0, 1, 2, 2], [0, 2, 2, 0]
    lsb = [rng.integers(0, 1 << bits, (P, H, spY)).astype(np.uint16), rng.integers(0, 1 << bits, (P, H // 2, spUV)).astype(np.uint16),
           None if nv12 else rng.integers(0, 1 << bits, (P, H // 2, spUV)).astype(np.uint16)]
    msb = [SC.msb_containers(a, bits, rng) if a is not None else None for a in lsb]
    assert np.all(msb[0] & ((1 << (16 - bits)) - 1))
    out = DeviceClip(*(to_dev(gpu, np.full(s, 7, np.uint16)) for s in ((4, H, pY), (4, H // 2, pUV), (4, H // 2, pUV))), width=W, height=H, bits=bits)
    dsrc = [to_dev(gpu, a) if a is not None else None for a in msb]
    weave_fields(gpu["ctx"], *dsrc, out, top, bot, nv12, msb=True)
    torch.cuda.synchronize()
    Y, U, V = lsb                                     # the oracle as it is, on the shifted pictures: the shift commutes with the copy
    for i in range(4):
        oY = np.full((H, pY), 7, np.uint16); oU = np.full((H // 2, pUV), 7, np.uint16); oV = np.full((H // 2, pUV), 7, np.uint16)
        t, b = top[i], bot[i]
        orc.lib.orc_merge_field(_ptr(Y[t]), _ptr(U[t]), _ptr(V[t]) if V is not None else None, _ptr(Y[b]), _ptr(U[b]),
                                _ptr(V[b]) if V is not None else None, spY, spUV, int(nv12), bits, W, H, _ptr(oY), _ptr(oU), _ptr(oV), pY, pUV)
        for g, o in ((out.Y[i], oY), (out.U[i], oU), (out.V[i], oV)):
            assert to_host(g, np.uint16).tobytes() == o.tobytes(), i


def test_weave_msb_refuses_8_bits(gpu):
    from amatsukaze_amd import AmtError, DeviceClip, weave_fields
    z = lambda *s: to_dev(gpu, np.zeros(s, np.uint8))
    out = DeviceClip(z(1, 8, 16), z(1, 4, 8), z(1, 4, 8), 16, 8, 8)
    with pytest.raises(AmtError, match="9..16"):
        weave_fields(gpu["ctx"], z(1, 8, 16), z(1, 4, 8), z(1, 4, 8), out, msb=True)


# ---- f. refusals: 0 with a message, nothing launched, the session stays usable ----
def test_refusals(gpu, orc, refdir, tmp_path):
    from amatsukaze_amd import binding
    lib, ctx = gpu["ctx"].lib, gpu["ctx"]
    W, H, lw, lh, x, y, n = K.geometry("A")
    want, _ = K.reference(orc, "A", 10, refdir)
    rng = np.random.default_rng(3)
    d = device_surfaces(gpu, SC.to_surfaces(K.clip("A", 10), 10, 1, 1, rng, 0, 0, 0xA5A5), W, H, 10, 1, 1)
    d8 = device_surfaces(gpu, SC.to_surfaces(small_clip(8), 8, 1, 0, rng, 0, 0, 0xA5), 64, 40, 8, 1, 0)
    dt = np.uint16
    sent = 0x5A5A
    outs = [to_dev(gpu, np.full(s, sent, dt)) for s in ((n, lh, lw), (n, lh // 2, lw // 2), (n, lh // 2, lw // 2))]

    def extract(desc, rect=(x, y, lw, lh), nframes=5):
        return lib.amtgpu_surfaces_extract_rect(ctx.h, C.byref(desc) if desc is not None else None, *rect, nframes,
                                                *(C.c_void_p(t.data_ptr()) for t in outs), lw * lh * 2, lw * lh // 2, lw, lw // 2)

    def changed(**kw):
        desc = d.ref()
        for k, v in kw.items():
            setattr(desc, k, v)
        return desc

    cx, wUV = x >> 1, lw >> 1
    planar = changed(interleaved=0)                      # (V is NULL in the P010 descriptor)
    for desc, rect, msg in ((changed(bits=8), None, b"9..16"),                           # msb_aligned at 8 bits
                            (changed(Y=None), None, b"null surface plane"), (changed(U=None), None, b"null surface plane"),
                            (planar, None, b"null surface plane"),                        # NULL V when planar
                            (changed(pitchUV=2 * (cx + wUV) - 1), None, b"pitchUV smaller"),
                            (changed(pitchY=x + lw - 1), None, b"pitchY smaller"),
                            (changed(reserved=1), None, b"reserved"), (changed(bits=17), None, b"8..16"),
                            (d.ref(), (x, y, lw - 1, lh), b"even-sized"), (d.ref(), (-2, y, lw, lh), b"even-sized")):
        assert extract(desc, rect or (x, y, lw, lh)) == 0, msg
        assert msg in last_error(gpu), (msg, last_error(gpu))
    assert extract(d.ref(), nframes=-1) == 0 and b"negative frame count" in last_error(gpu)
    assert extract(None) == 0 and b"null surface descriptor" in last_error(gpu)
    assert extract(d.ref(), nframes=0) == 1 and extract(None, nframes=0) == 1            # no frames: a no-op
    gpu["torch"].cuda.synchronize()
    assert all(np.all(to_host(t, dt) == sent) for t in outs), "a refused or empty call wrote to the destination"

    # the session
    st = lib.amtgpu_scanlogo_stream_create_bits(ctx.h, W, H, 10, x, y, lw, lh, THY, QUOTA)
    assert st
    nk, dn = C.c_int(-1), C.c_int(-1)

    def feed(desc, nframes):
        return lib.amtgpu_scanlogo_stream_feed_surfaces(st, C.byref(desc) if desc is not None else None, nframes, C.byref(nk), C.byref(dn))

    for desc, nframes, msg in ((d8.ref(), 5, b"another depth"), (changed(bits=12), 5, b"another depth"), (changed(Y=None), 5, b"null surface plane"),
                               (changed(U=None), 5, b"null surface plane"), (planar, 5, b"null surface plane"),
                               (changed(pitchUV=2 * (cx + wUV) - 1), 5, b"pitchUV smaller"), (changed(pitchY=x + lw - 1), 5, b"pitchY smaller"),
                               (d.ref(), -1, b"negative frame count"), (None, 5, b"null surface descriptor")):
        assert feed(desc, nframes) == 0, msg
        assert msg in last_error(gpu), (msg, last_error(gpu))
        assert (nk.value, dn.value) == (-1, -1)
    nr = C.c_int64(-1)
    assert feed(d.ref(), 0) == 1 and (nk.value, dn.value) == (0, 0)                     # no frames: returns 1, changes nothing
    assert lib.amtgpu_scanlogo_stream_status(st, C.byref(nr), None, None) == 1 and nr.value == 0
    # ... and the session is still good for the whole clip
    assert feed(d.ref(), n) == 1 and (nk.value, dn.value) == (QUOTA, 1), last_error(gpu)
    dst = tmp_path / "after_refusals.lgd"
    assert lib.amtgpu_scanlogo_stream_finish(st, SID, str(dst).encode(), binding.CB(lambda *a: 1)) == 1, last_error(gpu)
    assert dst.read_bytes() == want
    assert feed(d.ref(), 5) == 0 and b"finished" in last_error(gpu)                       # feed_surfaces after finish
    lib.amtgpu_scanlogo_stream_destroy(st)

    # the finder
    lf = lib.amtgpu_logofind_create(ctx.h, W, H, 10)
    assert lf
    for desc, nframes, msg in ((changed(bits=12), 5, b"another depth"), (changed(bits=8), 5, b"9..16"), (changed(Y=None), 5, b"null surface plane"),
                               (changed(pitchY=W - 1), 5, b"pitch below the width"), (d.ref(), -1, b"negative frame count")):
        assert lib.amtgpu_logofind_add_surfaces(lf, C.byref(desc), nframes) == 0, msg
        assert msg in last_error(gpu), (msg, last_error(gpu))
    assert lib.amtgpu_logofind_add_surfaces(lf, C.byref(d.ref()), 0) == 1 and lib.amtgpu_logofind_nframes(lf) == 0
    lib.amtgpu_logofind_destroy(lf)
    ctx.synchronize()
