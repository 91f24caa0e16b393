"""The cadence renderer on the GPU (amtgpu_kfm_render) against its numpy restatement (tests/kfm_render_ref.py):
every destination byte of the three planes, padding and the gaps between frames included, on both kernel forms, at 8, 10 and 16 bits,
with all three plan kinds, the clip-end clamps, planted threshold pixels, a clip cut into batches, the synthetic generator's film
pictures, and every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import kfm_render_ref as R

pytestmark = pytest.mark.gpu

W_, T_, B_ = R.WEAVE, R.BOB_TOP, R.BOB_BOTTOM
SENTINEL = 0xA5

# name: (width, height, bits, pitchY, pitchUV, gapY, gapUV)   pitches and the gap behind a frame's last row in containers
SHAPES = {
    "96x36-8-aligned": (96, 36, 8, 96, 48, 0, 0),
    "90x38-8-tail": (90, 38, 8, 96, 48, 0, 0),                  # 10-byte tail, chroma width 45, 19 chroma rows: the last has no row below
    "90x38-8-element": (90, 38, 8, 91, 46, 3, 1),               # pitch 91, frame strides 3461 / 875 bytes
    "1100x8-8-long-rows": (1100, 8, 8, 1104, 560, 0, 0),        # rows longer than the 1 024 bytes a wave covers per round
    "530x8-16-long-rows": (530, 8, 16, 536, 272, 0, 0),
    "96x36-10-aligned": (96, 36, 10, 96, 48, 0, 0),
    "90x38-10-tail": (90, 38, 10, 96, 48, 0, 0),                # 4-byte luma tail, 10-byte chroma tail
    "96x36-16-aligned": (96, 36, 16, 96, 48, 0, 0),
    "90x38-16-element": (90, 38, 16, 91, 46, 1, 1),             # frame strides 6918 / 1750 bytes
}
NSRC = 8
THRESHOLDS = (-1, 0, 3, 65535)


def all_kinds_plan(n):
    """all three kinds; WEAVE with top != bottom in both orders; the clip-end clamps BOB_TOP(0) and BOB_BOTTOM(n - 1); both bobs mid-clip"""
    return R.plan_array([(W_, 0, 0, 2), (W_, 3, 2, 2), (W_, 2, 3, 2), (T_, 0, 0, 1), (B_, n - 1, n - 1, 1), (T_, 4, 4, 1), (B_, 4, 4, 1),
                         (T_, n - 1, n - 1, 1), (B_, 0, 0, 1), (W_, 5, 5, 2)])


class HostClip:
    """planes of a clip as flat numpy buffers with pitches and frame gaps; .planes: the tight [n, h, w] views the reference reads"""

    def __init__(self, n, shape, fill=None, rng=None):
        self.w, self.h, self.bits, pY, pUV, gY, gUV = shape
        self.n = n
        self.dt = np.uint8 if self.bits <= 8 else np.uint16
        self.geom = [(self.h, self.w, pY, self.h * pY + gY), (self.h // 2, self.w // 2, pUV, (self.h // 2) * pUV + gUV)] * 2
        self.geom = [self.geom[0], self.geom[1], self.geom[1]]
        self.flat = []
        for rows, cols, pitch, fs in self.geom:
            if rng is not None:
                self.flat.append(rng.integers(0, 1 << (8 if self.bits <= 8 else 16 if self.bits == 16 else self.bits), n * fs).astype(self.dt))
            else:
                self.flat.append(np.full(n * fs, fill, self.dt))

    def view(self, k, flat=None):
        rows, cols, pitch, fs = self.geom[k]
        a = self.flat[k] if flat is None else flat
        es = a.itemsize
        return np.lib.stride_tricks.as_strided(a, (self.n, rows, pitch), (fs * es, pitch * es, es))

    @property
    def planes(self):
        return tuple(self.view(k)[:, :, :self.geom[k][1]] for k in range(3))


def plant(clip, thresh):
    """known pixels in the luma plane of frames 3..5 (BOB_TOP(4) fills row 5 from rows 4 / 6 and frames 3 / 4; BOB_BOTTOM(4) fills row 6
    from rows 5 / 7 and frames 4 / 5)"""
    Y = clip.planes[0]
    top = 255 if clip.bits <= 8 else 65535
    t = max(0, min(thresh, top - 101))
    # temporal neighbours that differ by exactly t (column 8 / 12) and by t + 1 (column 9 / 13); the spatial value is far away
    Y[4, 4, 8:10] = 200; Y[4, 6, 8:10] = 200
    Y[3, 5, 8:10] = 100; Y[4, 5, 8] = 100 + t; Y[4, 5, 9] = 100 + t + 1
    Y[4, 5, 12:14] = 220; Y[4, 7, 12:14] = 220
    Y[4, 6, 12:14] = 50; Y[5, 6, 12] = 50 + t; Y[5, 6, 13] = 50 + t + 1
    # the largest container next to 0, next to the largest but one and next to itself: as vertical neighbours (columns 20..22, whose
    # temporal neighbours differ by the whole range) and as temporal neighbours (columns 24..26, whose vertical neighbours give 8)
    Y[4, 4, 20:23] = top; Y[4, 6, 20:23] = (0, top - 1, top); Y[3, 5, 20:23] = 0; Y[4, 5, 20:23] = top
    Y[3, 5, 24:27] = top; Y[4, 5, 24:27] = (top - 1, 0, top); Y[4, 4, 24:27] = 7; Y[4, 6, 24:27] = 8
    if clip.bits == 10:
        Y[4, 4, 30] = 0xFFFF; Y[4, 6, 30] = 0x0401; Y[2, 1, 3] = 0xFC00         # containers beyond 10 bits: taken as stored
    return t


@functools.lru_cache(maxsize=None)
def source_clip(name, thresh):
    clip = HostClip(NSRC, SHAPES[name], rng=np.random.default_rng(sum(map(ord, name)) * 7 + 1))
    t = plant(clip, thresh)
    for a in clip.flat:
        a.setflags(write=False)
    return clip, t


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    ctx = Context(0)
    yield ctx, torch
    ctx.close()


def upload(gpu, clip, flats=None):
    """(DeviceSurfaces over device copies of the clip's flat buffers, the flat device tensors)"""
    ctx, torch = gpu
    from amatsukaze_amd import DeviceSurfaces
    dev = torch.device("cuda:0")
    flat_t, views = [], []
    for k, a in enumerate(flats or clip.flat):
        host = np.array(a, copy=True)
        t = torch.from_numpy(host if clip.bits <= 8 else host.view(np.int16)).to(dev)
        rows, cols, pitch, fs = clip.geom[k]
        flat_t.append(t)
        views.append(torch.as_strided(t, (clip.n, rows, pitch), (fs, pitch, 1)))
    return DeviceSurfaces(views[0], views[1], views[2], clip.w, clip.h, clip.bits), flat_t


def download(clip, flat_t):
    return [t.cpu().numpy().view(clip.dt) for t in flat_t]


def expected_buffers(dst, rendered):
    """the destination's flat buffers: the sentinel everywhere but in the rows' first `width` samples"""
    out = []
    for k in range(3):
        a = np.array(dst.flat[k], copy=True)
        dst.view(k, a)[:, :, :dst.geom[k][1]] = rendered[k]
        out.append(a)
    return out


def sentinel_clip(n, shape):
    bits = shape[2]
    return HostClip(n, shape, fill=SENTINEL if bits <= 8 else SENTINEL * 0x0101)


@pytest.mark.parametrize("thresh", THRESHOLDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_plane_byte_matches_the_reference(gpu, name, thresh):
    from amatsukaze_amd import kfm_render
    ctx, torch = gpu
    clip, t = source_clip(name, thresh)
    plan = all_kinds_plan(NSRC)
    want = R.render_ref(clip.planes, plan, thresh)
    # the planted pixels are what they were planted for (outputs 5 and 6 are BOB_TOP(4) and BOB_BOTTOM(4))
    top = 255 if clip.bits <= 8 else 65535
    Yw = want[0].astype(np.int64)
    if thresh < 0:
        assert Yw[5, 5, 8] == Yw[5, 5, 9] == 200 and Yw[6, 6, 12] == Yw[6, 6, 13] == 220
    elif thresh < top:
        assert Yw[5, 5, 8] == (200 + t + 1) >> 1 and Yw[5, 5, 9] == 200 and Yw[6, 6, 12] == (100 + t + 1) >> 1 and Yw[6, 6, 13] == 220
    else:
        assert Yw[5, 5, 9] == (200 + t + 2) >> 1 and Yw[6, 6, 13] == (100 + t + 2) >> 1                      # always temporal
    half = (top + 1) >> 1
    assert list(Yw[5, 5, 20:23]) == ([half] * 3 if thresh >= top else [half, top, top])                      # 17-bit sums
    assert list(Yw[5, 5, 24:27]) == ([8, 8, 8] if thresh < 0 else [top if thresh >= 1 else 8, half if thresh >= top else 8, top])
    assert list(Yw[6, 5, 20:23]) == [top] * 3                                                                 # a kept row

    src, src_flat = upload(gpu, clip)
    dst_host = sentinel_clip(len(plan), SHAPES[name])
    dst, dst_flat = upload(gpu, dst_host)
    kfm_render(ctx, src, plan, dst, thresh=thresh)
    torch.cuda.synchronize()
    got = download(dst_host, dst_flat)
    for k, (g, e) in enumerate(zip(got, expected_buffers(dst_host, want))):
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, (name, thresh, "plane", k, "first differing element", int(bad[0]), int(g[bad[0]]), int(e[bad[0]]))
    for g, a in zip(download(clip, src_flat), clip.flat):
        assert np.array_equal(g, a)                                                                            # the sources are unchanged


def test_a_clip_cut_into_batches_gives_the_bytes_of_one_call(gpu):
    from amatsukaze_amd import DeviceSurfaces, kfm_render, kfm_render_plan
    ctx, torch = gpu
    shape = SHAPES["90x38-8-tail"]
    N, thresh = 12, 3
    clip = HostClip(N, shape, rng=np.random.default_rng(12))
    I, F, P = R.CAD_60I, R.CAD_24P, R.CAD_30P
    cad = [I, I, F, F, F, F, F, P, P, I, I, I]
    ph = [0, 0, 0, 1, 2, 3, 4, 0, 0, 0, 0, 0]
    plan = kfm_render_plan(cad, ph)
    assert [tuple(int(v) for v in e)[:3] for e in plan] == [(T_, 0, 0), (B_, 0, 0), (T_, 1, 1), (B_, 1, 1), (W_, 2, 2), (W_, 3, 3), (W_, 5, 4),
                                                             (W_, 6, 6), (W_, 7, 7), (W_, 8, 8), (T_, 9, 9), (B_, 9, 9), (T_, 10, 10), (B_, 10, 10),
                                                             (T_, 11, 11), (B_, 11, 11)]
    want = R.render_ref(clip.planes, plan, thresh)
    src, _ = upload(gpu, clip)
    dst_host = sentinel_clip(len(plan), shape)
    whole, whole_flat = upload(gpu, dst_host)
    kfm_render(ctx, src, plan, whole, thresh=thresh)
    # three calls: the batch that owns frames [lo, hi) carries one frame on either side as its halo
    parts, parts_flat = upload(gpu, dst_host)
    k0 = 0
    for lo, hi in ((0, 4), (4, 8), (8, 12)):
        own = [i for i, e in enumerate(plan) if lo <= e["top"] < hi]
        assert own == list(range(k0, k0 + len(own)))
        a, b = max(0, lo - 1), min(N, hi + 1)
        cut = lambda s, i, j: DeviceSurfaces(s.Y[i:j], s.U[i:j], s.V[i:j], s.width, s.height, s.bits)
        kfm_render(ctx, cut(src, a, b), plan[own], cut(parts, k0, k0 + len(own)), src_first=a, clip_frames=N, thresh=thresh)
        k0 += len(own)
    assert k0 == len(plan)
    torch.cuda.synchronize()
    one, three = download(dst_host, whole_flat), download(dst_host, parts_flat)
    for g1, g3, e in zip(one, three, expected_buffers(dst_host, want)):
        assert np.array_equal(g1, g3) and np.array_equal(g1, e)


def test_rendered_film_frames_are_the_generator_film_pictures(gpu):
    import amt_synth as S
    from amatsukaze_amd import kfm_render, kfm_render_plan
    ctx, torch = gpu
    W, H, seed, N = 96, 36, 0x5EED0003, 20                          # all inside scene 0 (97 frames)
    shape = (W, H, 8, 96, 48, 0, 0)
    clip = HostClip(N, shape, fill=0)
    for n in range(N):
        for k, p in enumerate(S.frame_planes_np(n, W, H, seed, 8, "24p")):
            clip.planes[k][n] = p.astype(np.uint8)
    plan = kfm_render_plan([R.CAD_24P] * N, [n % 5 for n in range(N)])
    assert len(plan) == 16 and [int(t) for t in plan["ticks"]] == [2, 3, 2, 3] * 4
    src, _ = upload(gpu, clip)
    dst_host = sentinel_clip(16, shape)
    dst, dst_flat = upload(gpu, dst_host)
    kfm_render(ctx, src, plan, dst)
    torch.cuda.synchronize()
    got = download(dst_host, dst_flat)
    for g, e in zip(got, expected_buffers(dst_host, R.render_ref(clip.planes, plan, -1))):
        assert np.array_equal(g, e)
    Y = dst_host.view(0, got[0])[:, :, :W]
    for g in range(4):
        film = S.frame_planes_np(2 * g + 1, W, H, seed, 8, "30p")[0].astype(np.uint8)
        assert np.array_equal(Y[4 * g + 2], film), g
        assert not np.array_equal(clip.planes[0][5 * g + 2], film) and not np.array_equal(clip.planes[0][5 * g + 3], film)      # combed in the source
        for k, n in ((0, 0), (1, 1), (3, 4)):
            assert np.array_equal(Y[4 * g + k], clip.planes[0][5 * g + n])


# ---- refusals ----
def raw_render(ctx, s, src_first, nsrc, clip_frames, w, h, plan, thresh, d, nout=None):
    """(return value, message) of the C call"""
    pl = np.ascontiguousarray(plan, R.RENDER_FRAME).reshape(-1)
    r = ctx.lib.amtgpu_kfm_render(ctx.h, C.byref(s), src_first, nsrc, clip_frames, w, h, pl.ctypes.data_as(C.c_void_p), len(pl) if nout is None else nout,
                                  thresh, C.byref(d))
    return r, ctx.lib.amtgpu_last_error(ctx.h).decode(errors="replace")


def test_refusals_launch_nothing(gpu):
    from amatsukaze_amd import AmtError, DeviceSurfaces, binding, kfm_render
    ctx, torch = gpu
    shape = SHAPES["96x36-8-aligned"]
    W, H, N = 96, 36, 6
    clip = HostClip(N, shape, rng=np.random.default_rng(5))
    src, src_flat = upload(gpu, clip)
    dst_host = sentinel_clip(4, shape)
    dst, dst_flat = upload(gpu, dst_host)
    s, d = src.ref(), dst.ref()
    plan = lambda *e: R.plan_array(list(e))
    ok = plan((W_, 0, 0, 2))

    def changed(desc, **kw):
        c = binding.Surfaces()
        C.memmove(C.byref(c), C.byref(desc), C.sizeof(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    mid = DeviceSurfaces(src.Y[2:5], src.U[2:5], src.V[2:5], W, H, 8).ref()            # frames 2..4 of a clip of 8
    cases = {
        # name: (arguments, words the message must hold: the shared source/destination rule's refusals by their phrase)
        "odd width": ((s, 0, N, N, W - 1, H, ok, -1, d), "even"),
        "odd height": ((s, 0, N, N, W, H - 1, ok, -1, d), "even"),
        "height below 4": ((s, 0, N, N, W, 2, ok, -1, d), "at least 4"),
        "kind 3": ((s, 0, N, N, W, H, plan((3, 0, 0, 2)), -1, d), "kind outside 0..2"),
        "kind -1": ((s, 0, N, N, W, H, plan((W_, 0, 0, 2), (-1, 0, 0, 2)), -1, d), "plan entry 1: kind outside 0..2"),
        "BOB_TOP with top != bottom": ((s, 0, N, N, W, H, plan((T_, 1, 2, 1)), -1, d), "top == bottom"),
        "BOB_BOTTOM with top != bottom": ((s, 0, N, N, W, H, plan((B_, 2, 1, 1)), -1, d), "top == bottom"),
        "top behind the batch": ((s, 0, N, N, W, H, plan((W_, N, 0, 2)), -1, d), "top frame 6 is outside the batch"),
        "bottom negative": ((s, 0, N, N, W, H, plan((W_, 0, -1, 2)), -1, d), "bottom frame -1 is outside the batch"),
        "top before src_first": ((mid, 2, 3, 8, W, H, plan((W_, 1, 2, 2)), -1, d), "top frame 1 is outside the batch"),
        "bottom behind src_first + nsrc": ((mid, 2, 3, 8, W, H, plan((W_, 2, 5, 2)), -1, d), "bottom frame 5 is outside the batch"),
        "BOB_TOP without frame n - 1": ((mid, 2, 3, 8, W, H, plan((T_, 2, 2, 1)), 0, d), "the temporal neighbour 1 "),
        "BOB_BOTTOM without frame n + 1": ((mid, 2, 3, 8, W, H, plan((B_, 4, 4, 1)), 5, d), "the temporal neighbour 5 "),
        "batch outside the clip": ((s, 3, N, N, W, H, plan((W_, 3, 3, 2)), -1, d), "does not lie inside the clip"),
        "destination is the source": ((s, 0, N, N, W, H, ok, -1, s), "overlaps the source's"),
        "destination luma inside the source's chroma": ((s, 0, N, N, W, H, ok, -1, changed(d, Y=s.U)), "overlaps the source's"),
        "destination one byte into the source": ((s, 0, N, N, W, H, ok, -1, changed(d, V=s.Y + s.strideY * N - 1)), "overlaps the source's"),
        "NV12 source": ((changed(s, interleaved=1, pitchUV=W), 0, N, N, W, H, ok, -1, d), "not in kind"),
        "NV12 destination": ((s, 0, N, N, W, H, ok, -1, changed(d, interleaved=1, pitchUV=W)), "not in kind"),
        "MSB-aligned source": ((changed(s, bits=10, msb_aligned=1), 0, N, N, W, H, ok, -1, changed(d, bits=10)), "not in kind"),
        "different depths": ((s, 0, N, N, W, H, ok, -1, changed(d, bits=10)), "differ in bits"),
        "source pitch below the row": ((changed(s, pitchY=W - 2), 0, N, N, W, H, ok, -1, d), "source: pitch smaller than the row"),
        "destination chroma pitch below the row": ((s, 0, N, N, W, H, ok, -1, changed(d, pitchUV=W // 2 - 1)), "destination: pitch smaller than the row"),
        "overlapping destination frames": ((s, 0, N, N, W, H, plan((W_, 0, 0, 2), (W_, 1, 1, 2)), -1, changed(d, strideY=H * 96 - 1)), "destination frames overlap each other"),
        "null plan": None,
        "negative source stride": ((changed(s, strideY=-s.strideY), 0, N, N, W, H, ok, -1, d), "source: negative frame stride"),
        "negative destination chroma stride": ((s, 0, N, N, W, H, ok, -1, changed(d, strideUV=-d.strideUV)), "destination: negative frame stride"),
    }
    for what, case in cases.items():
        if case is None:
            r = ctx.lib.amtgpu_kfm_render(ctx.h, C.byref(s), 0, N, N, W, H, None, 1, -1, C.byref(d))
            msg, words = ctx.lib.amtgpu_last_error(ctx.h).decode(errors="replace"), "null plan"
        else:
            r, msg = raw_render(ctx, *case[0])
            words = case[1]
        assert r == 0 and "[KFMRender]" in msg and words in msg, (what, msg)
    assert raw_render(ctx, s, 0, N, N, W, H, ok, -1, d, nout=-1)[0] == 0
    assert raw_render(ctx, s, 0, N, N, W, H, ok, 0, d, nout=0)[0] == 1                                # nothing to render: 1
    with pytest.raises(AmtError, match="KFMRender"):
        kfm_render(ctx, src, plan((T_, 1, 2, 1)), dst)
    with pytest.raises(AmtError):
        kfm_render(ctx, src, plan(*[(W_, 0, 0, 2)] * 5), dst)                                        # more output frames than dst holds
    torch.cuda.synchronize()
    for g, a in zip(download(dst_host, dst_flat), dst_host.flat):
        assert np.array_equal(g, a)                                                                  # still the sentinel, everywhere
    for g, a in zip(download(clip, src_flat), clip.flat):
        assert np.array_equal(g, a)
    # the neighbours refused above are not needed without a threshold, and at the clip's ends there are none to need
    assert raw_render(ctx, mid, 2, 3, 8, W, H, plan((T_, 2, 2, 1), (B_, 4, 4, 1)), -1, d)[0] == 1
    ends = DeviceSurfaces(src.Y[0:1], src.U[0:1], src.V[0:1], W, H, 8).ref()
    assert raw_render(ctx, ends, 0, 1, 1, W, H, plan((T_, 0, 0, 1), (B_, 0, 0, 1)), 0, d)[0] == 1
    torch.cuda.synchronize()
    want = R.render_ref(tuple(p[0:1] for p in clip.planes), plan((T_, 0, 0, 1), (B_, 0, 0, 1)), 0)
    got = download(dst_host, dst_flat)
    for k in range(3):
        assert np.array_equal(dst_host.view(k, got[k])[:2, :, :dst_host.geom[k][1]], want[k])
