"""The temporal noise reduction on the GPU (amtgpu_temporal_nr) against its numpy restatement
(tests/temporal_nr_ref.py, which tests/test_temporal_nr_host.py holds against the compiled reference): every destination byte of the
three planes, guard bytes behind the rows and around the frames included, on both kernel forms and both container sizes; every count of
passing frames; planted pixels whose byte depends on the order and the rounding of the sum; clip ends, short clips, a clip cut into
batches, and every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import temporal_nr_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


class Buf:
    """a clip as three flat buffers of containers: row y of frame f of plane k starts at container off[k] + f * fs[k] + y * pitch[k].
    tight_end: the last row of the last frame ends the buffer"""

    def __init__(self, n, w, h, bits, pitch, gap=(0, 0), off=(0, 0, 0), tight_end=False, fill=0):
        self.n, self.w, self.h, self.bits = n, w, h, bits
        self.dt = np.uint8 if bits <= 8 else np.uint16
        self.geom, self.flat = [], []
        for k in range(3):
            rows, cols, p, g = (h, w, pitch[0], gap[0]) if k == 0 else (h // 2, w // 2, pitch[1], gap[1])
            fs = rows * p + g
            size = off[k] + ((n - 1) * fs + (rows - 1) * p + cols if tight_end else n * fs)
            self.geom.append((rows, cols, p, fs, off[k]))
            self.flat.append(np.full(size, fill, self.dt))

    def view(self, k, flat=None):
        rows, cols, p, fs, off = self.geom[k]
        a = self.flat[k] if flat is None else flat
        es = a.itemsize
        return np.lib.stride_tricks.as_strided(a[off:], (self.n, rows, cols), (fs * es, p * es, es))

    def put(self, planes):
        for k in range(3):
            self.view(k)[...] = planes[k]
        return self


def aligned_layouts(w, h, bits):
    """(source, destination) layouts on which the kernel takes its 16-byte form: luma rows 16-byte aligned, chroma rows 8-byte aligned;
    the two differ in pitches and strides, and the destination has guard containers in front of, between and behind its frames"""
    es = 1 if bits <= 8 else 2
    up = lambda v, m: (v + m - 1) // m * m
    pY, pUV = up(w * es, 16) // es, up(w // 2 * es, 8) // es
    src = dict(pitch=(pY, pUV), tight_end=True)
    dst = dict(pitch=(pY + 16 // es, pUV + 8 // es), gap=(32 // es, 24 // es), off=(16 // es, 8 // es, 16 // es))
    return src, dst


def narrow_layouts(w, h, bits):
    """plane bases one container off and pitches that are no multiple of 16 bytes: the container-by-container form"""
    src = dict(pitch=(w + 1, w // 2 + 2), gap=(3, 1), off=(1, 1, 1), tight_end=True)
    dst = dict(pitch=(w + 3, w // 2 + 1), gap=(1, 5), off=(1, 3, 1))
    return src, dst


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    ctx = Context(0)
    yield ctx, torch
    ctx.close()


def upload(gpu, buf):
    """(DeviceSurfaces over device copies of the buffers, the flat device tensors)"""
    ctx, torch = gpu
    from amatsukaze_amd import DeviceSurfaces
    dev = torch.device("cuda:0")
    flat_t, views = [], []
    for k, a in enumerate(buf.flat):
        host = np.array(a, copy=True)
        t = torch.from_numpy(host if buf.bits <= 8 else host.view(np.int16)).to(dev)
        rows, cols, p, fs, off = buf.geom[k]
        flat_t.append(t)
        views.append(torch.as_strided(t, (buf.n, rows, cols), (fs, p, 1), off))
    return DeviceSurfaces(views[0], views[1], views[2], buf.w, buf.h, buf.bits), flat_t


def download(buf, flat_t):
    return [t.cpu().numpy().view(buf.dt) for t in flat_t]


def cut(s, i, j):
    from amatsukaze_amd import DeviceSurfaces
    return DeviceSurfaces(s.Y[i:j], s.U[i:j], s.V[i:j], s.width, s.height, s.bits)


def sentinel_buf(n, w, h, bits, layout):
    return Buf(n, w, h, bits, fill=SENTINEL if bits <= 8 else SENTINEL * 0x0101, **{k: v for k, v in layout.items() if k != "tight_end"})


def check_against(what, dst_host, got, want, nout=None):
    """every container of the destination's buffers: the expected frames in the rows' first `width` containers, the sentinel elsewhere"""
    for k in range(3):
        e = np.array(dst_host.flat[k], copy=True)
        dst_host.view(k, e)[:want[k].shape[0] if nout is None else nout] = want[k]
        bad = np.flatnonzero(got[k] != e)
        assert bad.size == 0, (what, "plane", k, bad.size, "containers differ; the first at", int(bad[0]), "got", int(got[k][bad[0]]), "want", int(e[bad[0]]))


def run_whole_clip(gpu, what, planes, bits, d, thr, il, layouts, want=None):
    """filters the whole clip in one call and compares every destination container; the sources must stay as they were"""
    from amatsukaze_amd import temporal_nr
    ctx, torch = gpu
    n, h, w = planes[0].shape
    sl, dl = layouts(w, h, bits)
    src_host = Buf(n, w, h, bits, **sl).put(planes)
    dst_host = sentinel_buf(n, w, h, bits, dl)
    src, src_flat = upload(gpu, src_host)
    dst, dst_flat = upload(gpu, dst_host)
    assert temporal_nr(ctx, src, dst, distance=d, threshold=thr, interlaced=il) == (0, n)
    torch.cuda.synchronize()
    if want is None:
        want = R.filter_clip(planes, d, thr, bits, il)
    check_against(what, dst_host, download(dst_host, dst_flat), want)
    for g, a in zip(download(src_host, src_flat), src_host.flat):
        assert np.array_equal(g, a), (what, "the source changed")


# ---- every count of passing frames ----
# (bits, threshold, d, frames, width, height)
COUNT_CASES = [(8, 1, 3, 12, 34, 8), (8, 3, 3, 12, 34, 8), (10, 1, 3, 12, 34, 8), (14, 1, 3, 12, 34, 8), (16, 2, 3, 12, 34, 8), (8, 2, 1, 10, 34, 8),
               (12, 4, 5, 24, 6, 4)]


@functools.lru_cache(maxsize=None)
def count_case(case):
    bits, thr, d, n, w, h = case
    planes = R.make_clip(n, w, h, bits, thr, np.random.default_rng(sum(case) * 13 + 5))
    for p in planes:
        p.setflags(write=False)
    want = R.filter_clip(planes, d, thr, bits)
    for a in want:
        a.setflags(write=False)
    return planes, want


@pytest.mark.parametrize("case", COUNT_CASES, ids=lambda c: "bits%d-thr%d-d%d-%dx%dx%d" % c)
def test_every_count_of_passing_frames(gpu, case):
    bits, thr, d, n, w, h = case
    planes, want = count_case(case)
    # the generator's conditions, before the GPU result is looked at
    assert set(np.unique(want[3])) == set(range(1, 2 * d + 2)), sorted(np.unique(want[3]))
    for k in range(3):
        changed = float(np.mean(want[k] != planes[k]))
        print(case, "plane", k, "changed %.1f %%" % (100 * changed))
        assert changed >= 0.05, (k, changed)
    run_whole_clip(gpu, case, planes, bits, d, thr, False, aligned_layouts, want)


# ---- shapes: 16-byte lanes with every tail, the narrow form, both chroma mappings ----
@functools.lru_cache(maxsize=None)
def shape_clip(w, h, bits, seed=0):
    planes = R.make_clip(8, w, h, bits, 1, np.random.default_rng(w * 131 + h * 7 + bits + seed))
    if bits == 10:
        planes[0][3, h - 1, w - 1] = 0xFC00                    # containers above maxv: taken as stored
        planes[1][4, 0, 0] = 0xFFFF
        planes[2][2, h // 2 - 1, w // 2 - 1] = 0x0400
    for p in planes:
        p.setflags(write=False)
    return planes


@pytest.mark.parametrize("interlaced", [False, True], ids=["progressive", "interlaced"])
@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("h", [4, 8, 12])
@pytest.mark.parametrize("w", [2, 6, 34, 66, 130])
def test_vector_lanes_with_every_tail(gpu, w, h, bits, interlaced):
    run_whole_clip(gpu, (w, h, bits, interlaced), shape_clip(w, h, bits), bits, 3, 1, interlaced, aligned_layouts)


@pytest.mark.parametrize("interlaced", [False, True], ids=["progressive", "interlaced"])
@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("h", [4, 12])
def test_the_narrow_form_on_unaligned_planes(gpu, h, bits, interlaced):
    run_whole_clip(gpu, (18, h, bits, interlaced), shape_clip(18, h, bits), bits, 3, 1, interlaced, narrow_layouts)


# ---- parameters ----
@pytest.mark.parametrize("thr", [0, 1, 3, 255])
@pytest.mark.parametrize("d", [0, 1, 3, 5])
def test_distances_and_thresholds(gpu, d, thr):
    planes = R.make_clip(13, 34, 8, 8, max(1, min(thr, 3)), np.random.default_rng(d * 17 + thr))
    run_whole_clip(gpu, (d, thr), planes, 8, d, thr, False, aligned_layouts)


@pytest.mark.parametrize("bits", [8, 10, 12, 14, 16])
def test_every_depth(gpu, bits):
    planes = R.make_clip(9, 34, 8, bits, 1, np.random.default_rng(bits))
    if bits == 16:
        planes[0][4, 2, 2:6] = 65535                              # the largest container in a still area: sums at the top of the range
        planes[0][:, 3, 8] = 65535
    run_whole_clip(gpu, bits, planes, bits, 3, 1, True, aligned_layouts)


def test_the_largest_distance(gpu):
    planes = R.make_clip(130, 4, 4, 8, 1, np.random.default_rng(63))
    want = R.filter_clip(planes, 63, 1, 8)
    assert int(want[3].max()) >= 64                              # counts the short windows never reach
    run_whole_clip(gpu, "d = 63", planes, 8, 63, 1, False, aligned_layouts, want)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7])
def test_short_clips_follow_the_clamp_rule(gpu, n):
    planes = R.make_clip(n, 34, 8, 8, 1, np.random.default_rng(n))
    run_whole_clip(gpu, ("clip_frames", n), planes, 8, 3, 1, False, aligned_layouts)


# ---- planted ties: the pixels whose byte depends on how the sum is formed ----
def tie_search(bits, d, rng, W=512, H=256):
    """a clip of 2 d + 1 frames whose centre frame has, at every pixel, exactly 2 d passing frames with samples that sum to d mod 2 d in
    Y, U and V (the mean ends in .5), under threshold 3 d.  Per 2 x 2 block one window frame is far away in all three planes.  In each
    plane the centre is `base`, the other passing frames are base + e with e uniform in -u .. u (u = 1 << (bits - 8)), but for the last
    of them, whose e in -(d - 1) .. d brings the sum to d mod 2 d: every frame stays within d u of the centre in each plane"""
    n, u = 2 * d + 1, 1 << (bits - 8)
    maxv = (1 << bits) - 1
    far = 50 * u
    bh, bw = H // 2, W // 2
    fail = rng.integers(0, 2 * d, (bh, bw))
    fail = fail + (fail >= d)                                   # any frame but the centre
    planes = []
    for scale in (2, 1, 1):
        hh, ww = bh * scale, bw * scale
        yy, xx = np.arange(hh)[:, None], np.arange(ww)[None, :]
        f = np.repeat(np.repeat(fail, scale, 0), scale, 1)
        g = np.where(f == n - 1, n - 2, n - 1)                 # the last passing frame (never the centre: d >= 1)
        base = rng.integers(d * u, maxv - d * u + 1, (hh, ww))
        e = rng.integers(-u, u + 1, (n, hh, ww))
        e[d] = 0
        e[f, yy, xx] = 0
        e[g, yy, xx] = 0
        r = (d - e.sum(axis=0)) % (2 * d)
        e[g, yy, xx] = np.where(r <= d, r, r - 2 * d)
        P = base[None] + e
        P[f, yy, xx] = np.where(base + far <= maxv, base + far, base - far)
        assert P.min() >= 0 and P.max() <= maxv
        planes.append(P.astype(np.uint8 if bits <= 8 else np.uint16))
    return tuple(planes)


@functools.lru_cache(maxsize=None)
def tie_clip(bits, d, thr, w=66, h=8):
    """a small clip assembled from the 2 x 2 blocks of tie_search's clip in which a wrong variant gives another byte:
    (planes, reference output, {variant: pixels of the centre frame where it differs from the reference})"""
    rng = np.random.default_rng(bits * 100 + d)
    S = tie_search(bits, d, rng)
    ref = R.filter_frame(S, d, d, thr, bits)
    assert np.all(ref[3] == 2 * d)
    flags = {}
    for v in ("reversed", "rational", "fma"):
        o = R.filter_frame(S, d, d, thr, bits, variant=v)
        dy = o[0] != ref[0]
        flags[v] = dy[0::2, 0::2] | dy[0::2, 1::2] | dy[1::2, 0::2] | dy[1::2, 1::2] | (o[1] != ref[1]) | (o[2] != ref[2])
    nb = (w // 2) * (h // 2)
    chosen = []
    for v in ("reversed", "rational", "fma"):                      # the rarest first, a third of the blocks each
        ys, xs = np.nonzero(flags[v])
        chosen += [(int(y), int(x)) for y, x in zip(ys, xs)][:nb // 3]
    chosen = (chosen + [(y, x) for y in range(h // 2) for x in range(w // 2)])[:nb]         # the rest: any blocks
    by = np.array([c[0] for c in chosen]).reshape(h // 2, w // 2)
    bx = np.array([c[1] for c in chosen]).reshape(h // 2, w // 2)
    Y = np.empty((2 * d + 1, h, w), S[0].dtype)
    for dy in (0, 1):
        for dx in (0, 1):
            Y[:, dy::2, dx::2] = S[0][:, 2 * by + dy, 2 * bx + dx]
    planes = (Y, S[1][:, by, bx], S[2][:, by, bx])
    want = R.filter_clip(planes, d, thr, bits)
    differ = {}
    for v in ("reversed", "rational", "fma"):
        o = R.filter_frame(planes, d, d, thr, bits, variant=v)
        differ[v] = sum(int(np.sum(o[k] != want[k][d])) for k in range(3))
    return planes, want, differ


# the FMA variant must tell at every depth, the other two at 8 bits with count 6; elsewhere what the search found is reported
TIE_CASES = [(8, 3), (10, 3), (14, 3), (16, 3), (8, 5), (16, 5)]


@pytest.mark.parametrize("bits, d", TIE_CASES)
def test_planted_ties(gpu, bits, d):
    thr = 3 * d                                                  # tie_search's clips need it
    planes, want, differ = tie_clip(bits, d, thr)
    assert np.all(want[3][d] == 2 * d)                           # count 6 (10) at every pixel of the centre frame
    for k in range(3):                                           # whose samples sum to 3 mod 6 (5 mod 10) in every plane
        P = planes[k].astype(np.int64)
        assert np.all(np.sum(P * (np.abs(P - P[d]) <= d << (bits - 8)), axis=0) % (2 * d) == d)
    print("bits", bits, "count", 2 * d, "pixels of the centre frame where a wrong variant's byte differs:", differ)
    assert differ["fma"] >= 8, differ
    if bits == 8 and d == 3:
        assert differ["rational"] >= 8 and differ["reversed"] >= 8, differ
    else:
        for v in ("rational", "reversed"):
            if differ[v] < 8:
                print("  condition dropped at %d bits, count %d: the search found %d pixels for the %s variant" % (bits, 2 * d, differ[v], v))
    run_whole_clip(gpu, ("ties", bits, d), planes, bits, d, thr, False, aligned_layouts, want)


# ---- a clip cut into batches ----
def test_batches_with_halos_give_the_bytes_of_one_call(gpu):
    from amatsukaze_amd import temporal_nr
    ctx, torch = gpu
    N, w, h, bits, d, thr = 20, 34, 8, 8, 3, 1
    planes = R.make_clip(N, w, h, bits, thr, np.random.default_rng(20))
    want = R.filter_clip(planes, d, thr, bits)
    sl, dl = aligned_layouts(w, h, bits)
    src, _ = upload(gpu, Buf(N, w, h, bits, **sl).put(planes))
    dst_host = sentinel_buf(N, w, h, bits, dl)
    whole, whole_flat = upload(gpu, dst_host)
    parts, parts_flat = upload(gpu, dst_host)
    assert temporal_nr(ctx, src, whole, d, thr) == (0, N)
    for lo in range(0, N, 6):
        hi = min(N, lo + 6)
        a, b = max(0, lo - d), min(N, hi + d)
        # (a middle batch: the defaults are its own frames; the last batch's halo is the clip's end, whose frames the defaults would add)
        frames = {} if 0 < a and b < N else dict(out_first=lo, nout=hi - lo)
        assert temporal_nr(ctx, cut(src, a, b), cut(parts, lo, hi), d, thr, src_first=a, clip_frames=N, **frames) == (lo, hi - lo)
    torch.cuda.synchronize()
    one, many = download(dst_host, whole_flat), download(dst_host, parts_flat)
    check_against("one call", dst_host, one, want)
    for g1, g2 in zip(one, many):
        assert np.array_equal(g1, g2)


# ---- refusals ----
def test_refusals_launch_nothing(gpu):
    from amatsukaze_amd import AmtError, binding, temporal_nr
    ctx, torch = gpu
    N, w, h, bits = 8, 34, 8, 8
    planes = R.make_clip(N, w, h, bits, 1, np.random.default_rng(2))
    sl, dl = aligned_layouts(w, h, bits)
    src_host = Buf(N, w, h, bits, **sl).put(planes)
    src, src_flat = upload(gpu, src_host)
    dst_host = sentinel_buf(N, w, h, bits, dl)
    dst, dst_flat = upload(gpu, dst_host)
    s, t = src.ref(), dst.ref()
    mid = cut(src, 2, 6).ref()                                    # frames 2..5 of the clip of 8

    def changed(desc, **kw):
        c = binding.Surfaces()
        C.memmove(C.byref(c), C.byref(desc), C.sizeof(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def call(s_, src_first, nsrc, clip, w_, h_, out_first, nout, d, thr, il, t_):
        r = ctx.lib.amtgpu_temporal_nr(ctx.h, C.byref(s_), src_first, nsrc, clip, w_, h_, out_first, nout, d, thr, il, C.byref(t_))
        return r, ctx.lib.amtgpu_last_error(ctx.h).decode(errors="replace")

    es_pitchY = t.pitchY
    cases = {
        # name: (arguments, words the message must hold: the shared source/destination rule's refusals by their phrase)
        "temporal_distance -1": ((s, 0, N, N, w, h, 0, N, -1, 1, 0, t), "temporal_distance"),
        "temporal_distance 64": ((s, 0, N, N, w, h, 0, N, 64, 1, 0, t), "temporal_distance"),
        "threshold -1": ((s, 0, N, N, w, h, 0, N, 3, -1, 0, t), "threshold"),
        "threshold 32768": ((s, 0, N, N, w, h, 0, N, 3, 32768, 0, t), "threshold"),
        "bits 7": ((changed(s, bits=7), 0, N, N, w, h, 0, N, 3, 1, 0, changed(t, bits=7)), "bits"),
        "bits 17": ((changed(s, bits=17), 0, N, N, w, h, 0, N, 3, 1, 0, changed(t, bits=17)), "bits"),
        "different depths": ((s, 0, N, N, w, h, 0, N, 3, 1, 0, changed(t, bits=10)), "differ in bits"),
        "interleaved source": ((changed(s, interleaved=1), 0, N, N, w, h, 0, N, 3, 1, 0, t), "source: planar, LSB-aligned planes only"),
        "interleaved destination": ((s, 0, N, N, w, h, 0, N, 3, 1, 0, changed(t, interleaved=1)), "destination: planar, LSB-aligned planes only"),
        "MSB-aligned source": ((changed(s, bits=10, msb_aligned=1), 0, N, N, w, h, 0, N, 3, 1, 0, changed(t, bits=10)), "source: planar, LSB-aligned planes only"),
        "MSB-aligned destination": ((changed(s, bits=10), 0, N, N, w, h, 0, N, 3, 1, 0, changed(t, bits=10, msb_aligned=1)), "destination: planar, LSB-aligned planes only"),
        "odd width": ((s, 0, N, N, w - 1, h, 0, N, 3, 1, 0, t), "even"),
        "odd height": ((s, 0, N, N, w, h - 1, 0, N, 3, 1, 0, t), "even"),
        "interlaced with height % 4 == 2": ((s, 0, N, N, w, h - 2, 0, N, 3, 1, 1, t), "multiple of 4"),
        "source pitch below the row": ((changed(s, pitchY=w - 2), 0, N, N, w, h, 0, N, 3, 1, 0, t), "source: pitch smaller than the row"),
        "destination chroma pitch below the row": ((s, 0, N, N, w, h, 0, N, 3, 1, 0, changed(t, pitchUV=w // 2 - 1)), "destination: pitch smaller than the row"),
        "window frame before the batch": ((mid, 2, 4, N, w, h, 4, 1, 3, 1, 0, t), "window frame 1 "),
        "window frame behind the batch": ((mid, 2, 4, N, w, h, 5, 1, 1, 1, 0, t), "window frame 6 "),
        "batch outside the clip": ((s, 3, N, N, w, h, 3, 1, 0, 1, 0, t), "does not lie inside the clip"),
        "output frame behind the clip": ((s, 0, N, N, w, h, N - 1, 2, 0, 1, 0, t), "outside the clip"),
        "output frame before the clip": ((s, 0, N, N, w, h, -1, 2, 0, 1, 0, t), "outside the clip"),
        "negative output count": ((s, 0, N, N, w, h, 0, -1, 3, 1, 0, t), "negative"),
        "overlapping destination frames": ((s, 0, N, N, w, h, 0, 2, 3, 1, 0, changed(t, strideY=(h - 1) * es_pitchY + w - 1)), "destination frames overlap each other"),
        "destination is the source": ((s, 0, N, N, w, h, 0, N, 3, 1, 0, s), "overlaps the source's"),
        "destination luma inside the source's chroma": ((s, 0, N, N, w, h, 0, 1, 3, 1, 0, changed(t, Y=s.U)), "overlaps the source's"),
        "destination one byte into the source": ((s, 0, N, N, w, h, 0, 1, 3, 1, 0, changed(t, V=s.Y + s.strideY * (N - 1) + (h - 1) * s.pitchY + w - 1)), "overlaps the source's"),
        "negative source stride": ((changed(s, strideY=-s.strideY), 0, N, N, w, h, 0, N, 3, 1, 0, t), "source: negative frame stride"),
        "negative destination chroma stride": ((s, 0, N, N, w, h, 0, N, 3, 1, 0, changed(t, strideUV=-t.strideUV)), "destination: negative frame stride"),
    }
    for what, (args, words) in cases.items():
        r, msg = call(*args)
        assert r == 0 and msg.strip(), what
        assert "TemporalNR" in msg and words in msg, (what, msg)
    assert call(s, 0, N, N, w, h, 0, 0, 3, 1, 0, t)[0] == 1                                          # nothing to filter: 1
    with pytest.raises(AmtError, match="TemporalNR"):
        temporal_nr(ctx, src, dst, distance=64)
    with pytest.raises(AmtError):
        temporal_nr(ctx, src, cut(dst, 0, 3))                                                        # more output frames than dst holds
    torch.cuda.synchronize()
    for g, a in zip(download(dst_host, dst_flat), dst_host.flat):
        assert np.array_equal(g, a)                                                                  # still the sentinel, everywhere
    for g, a in zip(download(src_host, src_flat), src_host.flat):
        assert np.array_equal(g, a)
    # what the window refusals above lacked is all there at d = 1: frames 3 and 4 from the batch 2..5
    assert call(mid, 2, 4, N, w, h, 3, 2, 1, 1, 0, t)[0] == 1
    torch.cuda.synchronize()
    want = R.filter_clip(planes, 1, 1, bits, frames=[3, 4])
    check_against("frames 3 and 4", dst_host, download(dst_host, dst_flat), want)
