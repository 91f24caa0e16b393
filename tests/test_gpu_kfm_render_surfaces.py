"""The cadence renderer on decoder surfaces on the GPU (amtgpu_kfm_render with NV12 / P010 / P012 / planar MSB descriptors, source and
destination in kind) against its numpy restatement (tests/kfm_render_surfaces_ref.py): every destination byte,
padding and the gaps between frames included, on all six kernel forms, with planted pixels that tell a kernel that compares or rounds
containers from one that works on samples, clips cut into batches, the route through weave_fields and the planar kernel, and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import kfm_render_ref as R
import kfm_render_surfaces_ref as S
from test_gpu_kfm_render import SENTINEL, all_kinds_plan, gpu, raw_render  # noqa: F401  (gpu: the module's context fixture)

pytestmark = pytest.mark.gpu

W_, T_, B_ = R.WEAVE, R.BOB_TOP, R.BOB_BOTTOM

# name: (width, height, bits, interleaved, msb, pitchY, pitchUV, gapY, gapUV, one_allocation)   pitches and the gap behind a frame's last
# row in containers; one_allocation: Y and UV of a frame lie behind each other and both strides are the surface size
SHAPES = {
    "nv12-96x36-aligned": (96, 36, 8, True, False, 96, 96, 0, 0, False),
    "nv12-90x38-tail": (90, 38, 8, True, False, 96, 96, 0, 0, False),              # 10-byte luma and UV tails; 19 chroma rows: the last has no row below
    "nv12-90x38-element": (90, 38, 8, True, False, 91, 91, 3, 1, False),
    "nv12-1100x8-long-rows": (1100, 8, 8, True, False, 1104, 1104, 0, 0, False),    # a UV row longer than the 1 024 bytes a wave covers per round
    "nv12-96x36-one-allocation": (96, 36, 8, True, False, 96, 96, 0, 0, True),
    "p010-96x36-aligned": (96, 36, 10, True, True, 96, 96, 0, 0, False),
    "p010-90x38-tail": (90, 38, 10, True, True, 96, 96, 0, 0, False),               # 4-byte tails
    "p010-90x38-element": (90, 38, 10, True, True, 91, 91, 1, 1, False),
    "p010-530x8-long-rows": (530, 8, 10, True, True, 536, 536, 0, 0, False),
    "p012-96x36": (96, 36, 12, True, True, 96, 96, 0, 0, False),
    "p016-96x36-msb-flag-without-shift": (96, 36, 16, True, True, 96, 96, 0, 0, False),
    "interleaved-lsb-10-90x38": (90, 38, 10, True, False, 96, 96, 0, 0, False),
    "planar-msb-10-90x38": (90, 38, 10, False, True, 96, 48, 0, 0, False),
}
NSRC = 8
THRESHOLDS = (-1, 0, 3, "maxv")


class Surf:
    """a clip of surfaces as flat numpy buffers with pitches and frame gaps; .planes: the tight [n, rows, cols] container views -- (Y, UV)
    interleaved, (Y, U, V) planar"""

    def __init__(self, n, shape, fill=None, rng=None):
        self.w, self.h, self.bits, self.interleaved, self.msb, pY, pUV, gY, gUV, self.one = shape
        self.n, self.shape = n, shape
        self.dt = np.uint8 if self.bits <= 8 else np.uint16
        self.s = S.shift_of(self.bits, self.msb)
        self.top = (1 << self.bits) - 1 if self.s else 255 if self.bits <= 8 else 65535      # the largest sample the rule can meet
        hc, wc = self.h // 2, self.w if self.interleaved else self.w // 2
        sizes = [self.h * pY + gY] + [hc * pUV + gUV] * (1 if self.interleaved else 2)
        # per plane: (buffer, offset, rows, cols, pitch, frame stride), in containers
        if self.one:
            assert self.interleaved
            whole = sum(sizes)
            self.geom = [(0, 0, self.h, self.w, pY, whole), (0, sizes[0], hc, wc, pUV, whole)]
            lengths = [n * whole]
        else:
            self.geom = [(k, 0, (self.h, hc, hc)[k], (self.w, wc, wc)[k], (pY, pUV, pUV)[k], fs) for k, fs in enumerate(sizes)]
            lengths = [n * fs for fs in sizes]
        rand_top = 256 if self.bits <= 8 else 1 << 16 if self.msb else 1 << self.bits        # MSB: random low bits too
        self.flat = [rng.integers(0, rand_top, m).astype(self.dt) if rng is not None else np.full(m, fill, self.dt) for m in lengths]

    def view(self, k, flats=None):
        buf, off, rows, cols, pitch, fs = self.geom[k]
        a = (self.flat if flats is None else flats)[buf]
        es = a.itemsize
        return np.lib.stride_tricks.as_strided(a[off:], (self.n, rows, pitch), (fs * es, pitch * es, es))

    @property
    def planes(self):
        return tuple(self.view(k)[:, :, :g[3]] for k, g in enumerate(self.geom))


def sentinel_surf(n, shape):
    return Surf(n, shape, fill=SENTINEL if shape[2] <= 8 else SENTINEL * 0x0101)


def plant(c, thresh):
    """known pixels in frames 3..5.  BOB_TOP(4) (output 5 of all_kinds_plan) fills luma row 5 from rows 4 / 6 of frame 4 and from row 5 of
    frames 3 / 4; BOB_BOTTOM(4) (output 6) keeps row 5 of frame 4.  v(x) = x << s is a sample's container with zero low bits, low = the
    low bits all set"""
    Y = c.planes[0]
    s, top, low = c.s, c.top, (1 << c.s) - 1
    v = lambda x: x << s
    t = max(0, min(top if thresh == "maxv" else thresh, top - 101))
    Y[4, 4, 8:12] = v(200); Y[4, 6, 8:12] = v(200)
    # column 8: equal samples, different low bits (within thresh 0); 9: samples t + 1 apart, the smaller one with all its low bits set
    # (their containers are less than (t + 1) << s apart); 10: samples t apart, the larger one with all its low bits set (their containers
    # are more than t << s apart); 11: samples t + 1 apart, low bits zero
    Y[3, 5, 8:12] = (v(100) | low, v(100) | low, v(100), v(100))
    Y[4, 5, 8:12] = (v(100), v(100 + t + 1), v(100 + t) | low, v(100 + t + 1))
    # columns 14 / 15: samples 100 / 101 as temporal neighbours over 7 / 8 as vertical ones, low bits zero: both means round at the sample's unit
    Y[4, 4, 14:16] = v(7); Y[4, 6, 14:16] = v(8); Y[3, 5, 14:16] = v(100); Y[4, 5, 14:16] = v(101)
    # the largest sample next to 0 and next to itself: as vertical neighbours (columns 20 / 21, temporal neighbours the whole range apart)
    # and as temporal neighbours (columns 24 / 25, vertical neighbours giving 8); low bits set wherever there are any
    Y[4, 4, 20:22] = v(top) | low; Y[4, 6, 20:22] = (0, v(top) | low); Y[3, 5, 20:22] = low; Y[4, 5, 20:22] = v(top) | low
    Y[3, 5, 24:26] = v(top) | low; Y[4, 5, 24:26] = (low, v(top)); Y[4, 4, 24:26] = v(7) | low; Y[4, 6, 24:26] = v(8)
    # chroma pair 4 of row 1: U's temporal neighbours are equal samples, the V next to it has them the whole range apart
    if c.interleaved:
        UV = c.planes[1]
        u, w = (UV, 8), (UV, 9)
    else:
        u, w = (c.planes[1], 4), (c.planes[2], 4)
    for (P, x), a, b, vert in ((u, v(120) | low, v(120), v(40)), (w, low, v(top), v(60) | low)):
        P[4, 0, x] = vert; P[4, 2, x] = vert; P[3, 1, x] = a; P[4, 1, x] = b
    return t


@functools.lru_cache(maxsize=None)
def source(name, thresh):
    c = Surf(NSRC, SHAPES[name], rng=np.random.default_rng(sum(map(ord, name)) * 5 + 3))
    t = plant(c, thresh)
    for a in c.flat:
        a.setflags(write=False)
    return c, t


def upload(gpu, c, flats=None):
    """(DeviceSurfaces over device copies of the clip's flat buffers -- V None when interleaved --, the flat device tensors)"""
    ctx, torch = gpu
    from amatsukaze_amd import DeviceSurfaces
    dev = torch.device("cuda:0")
    flat_t = []
    for a in flats or c.flat:
        host = np.array(a, copy=True)
        flat_t.append(torch.from_numpy(host if c.bits <= 8 else host.view(np.int16)).to(dev))
    views = [torch.as_strided(flat_t[buf], (c.n, rows, pitch), (fs, pitch, 1), off) for buf, off, rows, cols, pitch, fs in c.geom]
    return DeviceSurfaces(views[0], views[1], None if c.interleaved else views[2], c.w, c.h, c.bits, c.interleaved, c.msb), flat_t


def download(c, flat_t):
    return [t.cpu().numpy().view(c.dt) for t in flat_t]


def expected_buffers(dst, rendered):
    """the destination's flat buffers: the sentinel everywhere but in the rows' first `cols` containers"""
    out = [np.array(a, copy=True) for a in dst.flat]
    for k, g in enumerate(dst.geom):
        dst.view(k, out)[:, :, :g[3]] = rendered[k]
    return out


def assert_buffers(got, want, *what):
    for k, (g, e) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, (*what, "buffer", k, "first differing element", int(bad[0]), int(g[bad[0]]), int(e[bad[0]]))


@functools.lru_cache(maxsize=None)
def restated(name, thresh):
    c, t = source(name, thresh)
    thr = c.top if thresh == "maxv" else thresh
    return S.render_surfaces_ref(c.planes, all_kinds_plan(NSRC), thr, c.bits, c.interleaved, c.msb)


def check_planted(c, t, thr, want):
    """the planted pixels are what they were planted for, on the restatement's output (outputs 5 and 6 are BOB_TOP(4) and BOB_BOTTOM(4))"""
    s, top, low = c.s, c.top, (1 << c.s) - 1
    Yc = want[0].astype(np.int64)
    Yw = Yc >> s
    row = list(Yw[5, 5, 8:12])
    if thr < 0:
        assert row == [200] * 4
    elif thr < top:
        assert row == [100, 200, (200 + t + 1) >> 1, 200]
    else:
        assert row == [100, (200 + t + 2) >> 1, (200 + t + 1) >> 1, (200 + t + 2) >> 1]                      # always temporal
    assert list(Yw[5, 5, 14:16]) == ([101, 101] if thr >= 1 else [8, 8])
    half = (top + 1) >> 1
    assert list(Yw[5, 5, 20:22]) == ([half] * 2 if thr >= top else [half, top])
    assert list(Yw[5, 5, 24:26]) == ([8, 8] if thr < 0 else [half if thr >= top else 8, top])
    assert not (Yc[5, 1::2] & low).any() and not (Yc[6, 0::2] & low).any()                                    # interpolated: zero low bits
    src_row = c.planes[0][4, 5].astype(np.int64)
    assert np.array_equal(Yc[6, 5], src_row) and np.array_equal(Yc[5, 4], c.planes[0][4, 4])                 # kept rows, as stored
    if s:
        assert Yc[6, 5, 10] & low == low and Yc[6, 5, 20] & low == low and Yc[5, 4, 24] & low == low          # ... their low bits survive
    if c.interleaved:
        UV = want[1].astype(np.int64)
        uv = [int(UV[5, 1, 8]) >> s, int(UV[5, 1, 9]) >> s]
        assert not (UV[5, 1, 8:10] & low).any()
    else:
        uv = [int(want[1][5, 1, 4]) >> s, int(want[2][5, 1, 4]) >> s]
    assert uv == ([40, 60] if thr < 0 else [120, half] if thr >= top else [120, 60])                          # the select does not span a U / V pair


@pytest.mark.parametrize("thresh", THRESHOLDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_surface_byte_matches_the_restatement(gpu, name, thresh):
    from amatsukaze_amd import kfm_render
    ctx, torch = gpu
    c, t = source(name, thresh)
    thr = c.top if thresh == "maxv" else thresh
    plan = all_kinds_plan(NSRC)
    want = restated(name, thresh)
    check_planted(c, t, thr, want)
    src, src_flat = upload(gpu, c)
    assert (src.V is None) == c.interleaved
    dst_host = sentinel_surf(len(plan), SHAPES[name])
    dst, dst_flat = upload(gpu, dst_host)
    kfm_render(ctx, src, plan, dst, thresh=thr)
    torch.cuda.synchronize()
    assert_buffers(download(dst_host, dst_flat), expected_buffers(dst_host, want), name, thresh)
    for g, a in zip(download(c, src_flat), c.flat):
        assert np.array_equal(g, a)                                                                            # the sources are unchanged


def cut(s, i, j):
    from amatsukaze_amd import DeviceSurfaces
    return DeviceSurfaces(s.Y[i:j], s.U[i:j], None if s.V is None else s.V[i:j], s.width, s.height, s.bits, s.interleaved, s.msb)


@pytest.mark.parametrize("name", ["nv12-90x38-tail", "p010-90x38-tail"])
def test_a_clip_cut_into_batches_gives_the_bytes_of_one_call(gpu, name):
    from amatsukaze_amd import kfm_render, kfm_render_plan
    ctx, torch = gpu
    shape = SHAPES[name]
    N, thresh = 12, 3
    c = Surf(N, shape, rng=np.random.default_rng(12))
    I, F, P = R.CAD_60I, R.CAD_24P, R.CAD_30P
    plan = kfm_render_plan([I, I, F, F, F, F, F, P, P, I, I, I], [0, 0, 0, 1, 2, 3, 4, 0, 0, 0, 0, 0])
    assert len(plan) == 16 and (W_, 5, 4) in [tuple(int(v) for v in e)[:3] for e in plan]
    want = S.render_surfaces_ref(c.planes, plan, thresh, c.bits, c.interleaved, c.msb)
    src, _ = upload(gpu, c)
    dst_host = sentinel_surf(len(plan), shape)
    whole, whole_flat = upload(gpu, dst_host)
    kfm_render(ctx, src, plan, whole, thresh=thresh)
    # three calls: the batch that owns frames [lo, hi) carries one frame on either side as its halo
    parts, parts_flat = upload(gpu, dst_host)
    k0 = 0
    for lo, hi in ((0, 4), (4, 8), (8, 12)):
        own = [i for i, e in enumerate(plan) if lo <= e["top"] < hi]
        assert own == list(range(k0, k0 + len(own)))
        a, b = max(0, lo - 1), min(N, hi + 1)
        kfm_render(ctx, cut(src, a, b), plan[own], cut(parts, k0, k0 + len(own)), src_first=a, clip_frames=N, thresh=thresh)
        k0 += len(own)
    assert k0 == len(plan)
    torch.cuda.synchronize()
    expect = expected_buffers(dst_host, want)
    assert_buffers(download(dst_host, whole_flat), expect, name, "one call")
    assert_buffers(download(dst_host, parts_flat), expect, name, "three calls")


def test_p010_render_is_the_planar_render_of_the_woven_samples(gpu):
    """the only route before: weave_fields(nv12=True, msb=True) planarises whole frames, the planar kernel renders them"""
    from amatsukaze_amd import DeviceClip, kfm_render, weave_fields
    ctx, torch = gpu
    shape, thresh = (90, 36, 10, True, True, 96, 96, 0, 0, False), 3          # (the weave wants a height that is a multiple of 4)
    c = Surf(NSRC, shape, rng=np.random.default_rng(10))
    plan = all_kinds_plan(NSRC)
    src, _ = upload(gpu, c)
    dst_host = sentinel_surf(len(plan), shape)
    dst, dst_flat = upload(gpu, dst_host)
    kfm_render(ctx, src, plan, dst, thresh=thresh)
    mk = lambda n, h, w: torch.zeros((n, h, w), dtype=torch.int16, device="cuda:0")
    planar = DeviceClip(mk(NSRC, c.h, c.w), mk(NSRC, c.h // 2, c.w // 2), mk(NSRC, c.h // 2, c.w // 2), c.w, c.h, c.bits)
    weave_fields(ctx, src.Y, src.U, None, planar, nv12=True, msb=True)
    out = DeviceClip(mk(len(plan), c.h, c.w), mk(len(plan), c.h // 2, c.w // 2), mk(len(plan), c.h // 2, c.w // 2), c.w, c.h, c.bits)
    kfm_render(ctx, planar, plan, out, thresh=thresh)
    torch.cuda.synchronize()
    got = download(dst_host, dst_flat)
    Y, UV = (dst_host.view(k, got)[:, :, :dst_host.geom[k][3]] for k in range(2))
    host = lambda t: t.cpu().numpy().view(np.uint16)
    assert np.array_equal(Y >> c.s, host(out.Y)) and np.array_equal(UV[:, :, 0::2] >> c.s, host(out.U)) and np.array_equal(UV[:, :, 1::2] >> c.s, host(out.V))
    # and the rest of the identity: copied rows as stored, interpolated containers with zero low bits
    low = (1 << c.s) - 1
    for k, e in enumerate(plan):
        for parity, frame in S.copied_rows(e, 0):
            assert np.array_equal(Y[k, parity::2], c.planes[0][frame, parity::2]) and np.array_equal(UV[k, parity::2], c.planes[1][frame, parity::2])
        ip = S.interpolated_rows(e)
        if ip is not None:
            assert not (Y[k, ip::2] & low).any() and not (UV[k, ip::2] & low).any()


def changed(desc, **kw):
    from amatsukaze_amd import binding
    c = binding.Surfaces()
    C.memmove(C.byref(c), C.byref(desc), C.sizeof(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_refusals_launch_nothing_and_null_v_is_accepted(gpu):
    ctx, torch = gpu
    N, NOUT = 4, 2
    ok = R.plan_array([(W_, 0, 0, 2), (W_, 1, 1, 2)])
    clips = {}

    def pair(name, shape):
        """source (random) and destination (sentinel) of a shape on the device: (host, DeviceSurfaces, flat tensors) each"""
        sh, dh = Surf(N, shape, rng=np.random.default_rng(len(name))), sentinel_surf(NOUT, shape)
        clips[name] = [(sh, *upload(gpu, sh)), (dh, *upload(gpu, dh))]
        return clips[name][0][1].ref(), clips[name][1][1].ref()

    W, H = 96, 36
    nv12_s, nv12_d = pair("nv12", SHAPES["nv12-96x36-one-allocation"])
    pl8_s, pl8_d = pair("planar8", (W, H, 8, False, False, 96, 48, 0, 0, False))
    p010_s, p010_d = pair("p010", SHAPES["p010-96x36-aligned"])
    il10_s, il10_d = pair("interleaved-lsb-10", (W, H, 10, True, False, 96, 96, 0, 0, False))
    p012_s, p012_d = pair("p012", SHAPES["p012-96x36"])
    pm10_s, pm10_d = pair("planar-msb-10", (W, H, 10, False, True, 96, 48, 0, 0, False))
    assert nv12_s.strideY == nv12_s.strideUV == W * H * 3 // 2 and nv12_s.U == nv12_s.Y + W * H and not nv12_s.V and not nv12_d.V
    cases = {
        # name: (source, destination, words the message must hold)
        # not in kind
        "NV12 into planes": (nv12_s, pl8_d, "not in kind"),
        "planes into NV12": (pl8_s, nv12_d, "not in kind"),
        "P010 into planar MSB": (p010_s, pm10_d, "not in kind"),
        "planar MSB into P010": (pm10_s, p010_d, "not in kind"),
        "P010 into interleaved LSB (shift 6 against 0)": (p010_s, il10_d, "converts no layouts"),
        "interleaved LSB into P010": (il10_s, p010_d, "converts no layouts"),
        "P010 into P012 (bits, and shift 6 against 4)": (p010_s, p012_d, "differ in bits"),
        "P012 into P010": (p012_s, p010_d, "differ in bits"),
        "P010 into a descriptor that says P012 of the same planes' layout": (p010_s, changed(p010_d, bits=12), "differ in bits"),
        # in kind, and refused all the same
        "interleaved source pitchUV below width": (changed(nv12_s, pitchUV=W - 2), nv12_d, "source: pitch smaller than the row"),
        "interleaved destination pitchUV below width": (nv12_s, changed(nv12_d, pitchUV=W - 2), "destination: pitch smaller than the row"),
        "destination Y inside the source's UV plane": (nv12_s, changed(nv12_d, Y=nv12_s.U), "overlaps the source's"),
        "destination UV over the source's Y plane": (nv12_s, changed(nv12_d, U=nv12_s.Y), "overlaps the source's"),
        "overlapping destination frames on the UV plane": (nv12_s, changed(nv12_d, strideUV=(H // 2) * 96 - 1), "destination frames overlap each other"),
        "negative source stride": (changed(p010_s, strideY=-p010_s.strideY), p010_d, "source: negative frame stride"),
        "negative destination UV stride": (nv12_s, changed(nv12_d, strideUV=-nv12_d.strideUV), "destination: negative frame stride"),
    }
    for what, (s, d, words) in cases.items():
        r, msg = raw_render(ctx, s, 0, N, N, W, H, ok, 0, d)
        assert r == 0 and "[KFMRender]" in msg and words in msg, (what, r, msg)
    torch.cuda.synchronize()
    for name, both in clips.items():
        for host, _, flat_t in both:
            for g, a in zip(download(host, flat_t), host.flat):
                assert np.array_equal(g, a), name                                   # sources as they were, destinations still the sentinel
    # accepted: interleaved with V = NULL on both sides, Y and UV of one allocation with both strides the surface size
    r, msg = raw_render(ctx, nv12_s, 0, N, N, W, H, ok, 0, nv12_d)
    assert r == 1, msg
    torch.cuda.synchronize()
    sh, dh = clips["nv12"][0][0], clips["nv12"][1][0]
    want = S.render_surfaces_ref(sh.planes, ok, 0, 8, True, False)
    assert_buffers(download(dh, clips["nv12"][1][2]), expected_buffers(dh, want), "NULL V")
    # ... and whatever V holds when interleaved is not looked at
    r, msg = raw_render(ctx, changed(p010_s, V=1), 0, N, N, W, H, ok, 3, changed(p010_d, V=3))
    assert r == 1, msg
    torch.cuda.synchronize()
    sh, dh = clips["p010"][0][0], clips["p010"][1][0]
    want = S.render_surfaces_ref(sh.planes, ok, 3, 10, True, True)
    assert_buffers(download(dh, clips["p010"][1][2]), expected_buffers(dh, want), "stray V")
