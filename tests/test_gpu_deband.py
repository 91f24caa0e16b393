"""The deband on the GPU (amtgpu_deband_*) against its numpy restatement (tests/deband_ref.py, which
tests/test_deband_host.py holds against the rule's text and the C++ tables): every destination container of the three planes, guard
containers behind the rows and around the frames included, on both kernel forms and both container sizes; planes smaller than any
radius, tiles that are all halo, an interior tile and chroma tiles of another shape; every radius, sample and blur_first; planted
tables that send every pixel to the outermost row and column of its tile's halo; containers whose sums need more than 16 bits; a clip
cut into calls; and every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import deband_ref as R
from test_gpu_temporal_nr import Buf, check_against, cut, download, narrow_layouts, sentinel_buf, upload

pytestmark = pytest.mark.gpu

# mirrored from csrc/kernels.hpp (tests/test_deband_host.py holds the line against the file)
TW, TH = 128, 96
SIZES = [(2, 2), (8, 6), (TW + 2, TH + 2), (2 * TW + 34, 2 * TH + 6)]
# (bits, bits of the content): 8-bit containers; 16-bit containers with 14-bit and with full 16-bit content
DEPTHS = [(8, 8), (14, 14), (16, 16)]
MODES = [(0, True), (1, True), (1, False), (2, True), (2, False)]     # (sample, blur_first); sample 0 has one form


def aligned_layouts(w, h, bits):
    """(source, destination) layouts on which the kernel takes its 16-byte form: every row of every plane 16-byte aligned; the two differ
    in pitches and strides, and the destination has guard containers in front of, between and behind its frames"""
    es = 1 if bits <= 8 else 2
    up = lambda v, m: (v + m - 1) // m * m
    pY, pUV = up(w * es, 16) // es, up(w // 2 * es, 16) // es
    src = dict(pitch=(pY, pUV), tight_end=True)
    dst = dict(pitch=(pY + 16 // es, pUV + 32 // es), gap=(32 // es, 48 // es), off=(16 // es, 32 // es, 16 // es))
    return src, dst


LAYOUTS = {"aligned": aligned_layouts, "one-off": narrow_layouts}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    ctx = Context(0)
    yield ctx, torch
    ctx.close()


@functools.lru_cache(maxsize=None)
def clip(w, h, depth, kind, n=2):
    """random: every container uniform over the content's range.  soft: a ramp in steps with noise of a few 8-bit units, on which a small
    threshold keeps some pixels and filters others"""
    bits, content = depth
    dt = np.uint8 if bits <= 8 else np.uint16
    rng = np.random.default_rng(w * 977 + h * 31 + content + (7 if kind == "soft" else 0))
    planes = []
    for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2)):
        if kind == "random":
            p = rng.integers(0, 1 << content, (n, ph, pw))
        else:
            u = 1 << (content - 8)
            p = (64 + (np.arange(pw)[None, None, :] // 16) * 2) * u + rng.integers(0, 4 * u + 1, (n, ph, pw))
        p = p.astype(dt)
        p.setflags(write=False)
        planes.append(p)
    return tuple(planes)


def run_case(gpu, what, planes, bits, layouts, want, offsets=None, **params):
    """one call over the whole clip: every destination container against `want`, the sources unchanged"""
    from amatsukaze_amd import Debander
    ctx, torch = gpu
    n, h, w = planes[0].shape
    sl, dl = layouts(w, h, bits)
    src_host = Buf(n, w, h, bits, **sl).put(planes)
    dst_host = sentinel_buf(n, w, h, bits, dl)
    src, src_flat = upload(gpu, src_host)
    dst, dst_flat = upload(gpu, dst_host)
    db = Debander(ctx, (w, h), bits, **params)
    if offsets is not None:
        for p, (dx, dy) in enumerate(offsets):
            db.set_offsets(p, dx, dy)
    assert db.run(src, dst) == n
    db.close()
    torch.cuda.synchronize()
    check_against(what, dst_host, download(dst_host, dst_flat), want)
    for g, a in zip(download(src_host, src_flat), src_host.flat):
        assert np.array_equal(g, a), (what, "the source changed")


# ---- every size, depth and lane form; under each every radius, sample and blur_first ----
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("depth", DEPTHS, ids=lambda d: "bits%d-content%d" % d)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_every_radius_sample_and_blur_first(gpu, size, depth, layout):
    w, h = size
    bits = depth[0]
    for radius in (1, 25, 31):
        offsets = R.tables(w, h, radius, seed=radius)
        soft_outputs = {}
        for sample, bf in MODES:
            # random content under the largest threshold: every gathered sample reaches the output; soft content under a small one:
            # the comparison decides
            for kind, threshold in (("random", 32767), ("soft", 2)):
                planes = clip(w, h, depth, kind)
                want = R.filter_clip(planes, bits, radius, threshold, sample, bf, offsets=offsets)
                if kind == "soft":
                    soft_outputs[(sample, bf)] = want
                run_case(gpu, (size, depth, layout, radius, sample, bf, kind), planes, bits, LAYOUTS[layout], want,
                         radius=radius, threshold=threshold, sample=sample, blur_first=bf, seed=radius)
        if w >= TW:
            # the cases were worth running: on the soft clip the threshold keeps some pixels and filters others, and the two blur_first
            # settings give other bytes
            soft = clip(w, h, depth, "soft")
            for sample in (1, 2):
                a, b = soft_outputs[(sample, True)][0], soft_outputs[(sample, False)][0]
                assert not np.array_equal(a, b), (radius, sample)
                assert 0.02 < np.mean(b != soft[0]) < 0.98, (radius, sample, float(np.mean(b != soft[0])))


# ---- planted tables: every pixel's references on the rim of what it may reach ----
DIRECTIONS = [(1, 1), (-1, 1), (1, 0), (0, -1)]                        # (dx, dy) in units of lim(x, y)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("depth", [(8, 8), (16, 16)], ids=lambda d: "bits%d" % d[0])
@pytest.mark.parametrize("size", SIZES[2:], ids=lambda s: "%dx%d" % s)
def test_planted_tables_read_the_outermost_halo(gpu, size, depth, layout):
    w, h = size
    bits = depth[0]
    planes = clip(w, h, depth, "random")
    for radius in (25, 31):
        for sx, sy in DIRECTIONS:
            offsets = []
            for p in range(3):
                lim = R.lim_map(*R.plane_size(p, w, h), R.plane_radius(p, radius))
                offsets.append(((sx * lim).astype(np.int8), (sy * lim).astype(np.int8)))
            # the four references of an interior pixel are then `radius` away in all four directions, and the first and last row and
            # column of every tile read the outermost row and column of its halo
            assert int(np.abs(offsets[0][0]).max() + np.abs(offsets[0][1]).max()) >= radius
            want = R.filter_clip(planes, bits, radius, 32767, 2, True, offsets=offsets)
            run_case(gpu, (size, bits, layout, radius, sx, sy), planes, bits, LAYOUTS[layout], want, offsets=offsets,
                     radius=radius, threshold=32767, sample=2, blur_first=True)


# ---- sums that need more than 16 bits ----
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("pattern", ["all-65535", "checkers", "coin-flips"])
def test_sums_of_four_large_containers(gpu, pattern, layout):
    w, h, n = TW + 2, TH + 2, 2
    planes, rng = [], np.random.default_rng(65535)
    for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2)):
        y, x = np.arange(ph)[None, :, None], np.arange(pw)[None, None, :]
        f = np.arange(n)[:, None, None]
        # (the four references of a pixel lie dx + dy, mod 2, from it: on checkers they are equal, four 65 535s or four zeros; the coin
        # flips give every count of 65 535s among them)
        p = {"all-65535": lambda: np.full((n, ph, pw), 65535), "checkers": lambda: ((x + y + f) & 1) * 65535,
             "coin-flips": lambda: rng.integers(0, 2, (n, ph, pw)) * 65535}[pattern]()
        planes.append(p.astype(np.uint16))
    planes = tuple(planes)
    for sample, bf in ((1, True), (2, True), (2, False)):
        for threshold in (32767, 0):
            want = R.filter_clip(planes, 16, 25, threshold, sample, bf, seed=3)
            if pattern == "checkers" and threshold:
                assert set(np.unique(want[0]).tolist()) == {0, 65535} and not np.array_equal(want[0], planes[0])
            if pattern == "coin-flips" and threshold and sample == 2:
                # 0 .. 4 containers of 65 535 among the four: (k * 65535 + 2) >> 2, 18 bits before the shift
                assert set(np.unique(want[0]).tolist()) == {0, 16384, 32768, 49151, 65535}
            run_case(gpu, (pattern, layout, sample, bf, threshold), planes, 16, LAYOUTS[layout], want,
                     radius=25, threshold=threshold, sample=sample, blur_first=bf, seed=3)


# ---- a clip cut into calls ----
@pytest.mark.parametrize("bits", [8, 14])
def test_calls_of_2_and_3_frames_give_the_bytes_of_one_call(gpu, bits):
    from amatsukaze_amd import Debander
    ctx, torch = gpu
    w, h, N = TW + 2, TH + 2, 5
    planes = clip(w, h, (bits, bits), "soft", N)
    want = R.filter_clip(planes, bits)                                  # the defaults: 25, 1, 2, true, seed 0
    sl, dl = aligned_layouts(w, h, bits)
    src, _ = upload(gpu, Buf(N, w, h, bits, **sl).put(planes))
    dst_host = sentinel_buf(N, w, h, bits, dl)
    whole, whole_flat = upload(gpu, dst_host)
    parts, parts_flat = upload(gpu, dst_host)
    db = Debander(ctx, (w, h), bits)
    assert db.run(src, whole) == N
    assert db.run(cut(src, 0, 2), cut(parts, 0, 2)) == 2 and db.run(cut(src, 2, 5), cut(parts, 2, 5)) == 3
    db.close()
    torch.cuda.synchronize()
    one, many = download(dst_host, whole_flat), download(dst_host, parts_flat)
    check_against("one call", dst_host, one, want)
    assert any(not np.array_equal(want[k], planes[k]) for k in range(3))
    for g1, g2 in zip(one, many):
        assert np.array_equal(g1, g2)


# ---- the tables ----
@pytest.mark.parametrize("size, radius, seed", [((2, 2), 31, 0), ((8, 6), 25, 1), ((TW + 2, TH + 2), 25, 0), ((2 * TW + 34, 2 * TH + 6), 31, 0xFFFFFFFF)])
def test_get_offsets_is_the_restatements_table(gpu, size, radius, seed):
    from amatsukaze_amd import Debander
    ctx, _ = gpu
    db = Debander(ctx, size, 10, radius, seed=seed)
    for p, (dx, dy) in enumerate(R.tables(*size, radius, seed)):
        gx, gy = db.offsets(p)
        assert gx.dtype == np.int8 and np.array_equal(gx, dx) and np.array_equal(gy, dy), (size, p)
    # a table that was set is the table that is read back
    lim = R.lim_map(*size, radius)
    db.set_offsets(0, (-lim).astype(np.int8), lim.astype(np.int8))
    gx, gy = db.offsets(0)
    assert np.array_equal(gx, -lim) and np.array_equal(gy, lim)
    db.close()


# ---- refusals ----
def test_refusals_write_nothing(gpu):
    from amatsukaze_amd import AmtError, Debander, binding
    ctx, torch = gpu
    N, w, h, bits, radius = 3, 34, 20, 8, 5
    planes = clip(w, h, (8, 8), "random", N)
    sl, dl = aligned_layouts(w, h, bits)
    src_host = Buf(N, w, h, bits, **sl).put(planes)
    src, src_flat = upload(gpu, src_host)
    dst_host = sentinel_buf(N, w, h, bits, dl)
    dst, dst_flat = upload(gpu, dst_host)
    s, t = src.ref(), dst.ref()
    lib = ctx.lib
    last = lambda: lib.amtgpu_last_error(ctx.h).decode(errors="replace")

    # create
    good = dict(width=w, height=h, bits=bits, radius=radius, threshold=1, sample=2, blur_first=1, seed=0)
    for what, kw in {"odd width": dict(width=w - 1), "odd height": dict(height=h - 1), "no width": dict(width=0), "negative height": dict(height=-2),
                     "width above 65534": dict(width=65536), "height above 65534": dict(height=65536), "bits 7": dict(bits=7), "bits 17": dict(bits=17),
                     "radius 0": dict(radius=0), "radius 32": dict(radius=32), "threshold -1": dict(threshold=-1), "threshold 32768": dict(threshold=32768),
                     "sample -1": dict(sample=-1), "sample 3": dict(sample=3)}.items():
        a = dict(good, **kw)
        handle = lib.amtgpu_deband_create(ctx.h, a["width"], a["height"], a["bits"], a["radius"], a["threshold"], a["sample"], a["blur_first"], a["seed"])
        assert not handle and "[Deband]" in last(), (what, last())
    with pytest.raises(AmtError, match="Deband"):
        Debander(ctx, (w, h), bits, radius=32)
    db = Debander(ctx, (w, h), bits, radius, 32767, 2, True)
    db10 = Debander(ctx, (w, h), 10, radius)

    def changed(desc, **kw):
        c = binding.Surfaces()
        C.memmove(C.byref(c), C.byref(desc), C.sizeof(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def call(obj, s_, t_, n):
        r = lib.amtgpu_deband_run(obj.h, C.byref(s_), C.byref(t_), n)
        return r, last()

    # run
    cases = {
        # name: (arguments..., words the message must hold)
        "interleaved source": (db, changed(s, interleaved=1), t, N, "source: planar, LSB-aligned planes only"),
        "interleaved destination": (db, s, changed(t, interleaved=1), N, "destination: planar, LSB-aligned planes only"),
        "MSB-aligned source": (db10, changed(s, bits=10, msb_aligned=1), changed(t, bits=10), N, "source: planar, LSB-aligned planes only"),
        "MSB-aligned destination": (db10, changed(s, bits=10), changed(t, bits=10, msb_aligned=1), N, "destination: planar, LSB-aligned planes only"),
        "bits that are not the object's": (db10, s, t, N, "source: 8 bits, the debander was created for 10"),
        "source of other bits": (db, changed(s, bits=10), t, N, "source: 10 bits, the debander was created for 8"),
        "destination of other bits": (db, s, changed(t, bits=10), N, "destination: 10 bits, the debander was created for 8"),
        "source pitch below the row": (db, changed(s, pitchY=w - 2), t, N, "source: pitch smaller than the row"),
        "destination chroma pitch below the row": (db, s, changed(t, pitchUV=w // 2 - 1), N, "destination: pitch smaller than the row"),
        "negative source stride": (db, changed(s, strideY=-s.strideY), t, N, "source: negative frame stride"),
        "negative destination chroma stride": (db, s, changed(t, strideUV=-t.strideUV), N, "destination: negative frame stride"),
        "negative frame count": (db, s, t, -1, "negative frame count"),
        "overlapping destination frames": (db, s, changed(t, strideY=(h - 1) * t.pitchY + w - 1), 2, "destination frames overlap each other"),
        "destination is the source": (db, s, s, N, "overlaps the source's"),
        "destination luma inside the source's chroma": (db, s, changed(t, Y=s.U), 1, "overlaps the source's"),
        "destination one byte into the source": (db, s, changed(t, V=s.Y + s.strideY * (N - 1) + (h - 1) * s.pitchY + w - 1), N, "overlaps the source's"),
        "null source plane": (db, changed(s, V=None), t, N, "null surface plane"),
    }
    for what, (*args, words) in cases.items():
        r, msg = call(*args)
        assert r == 0 and "[Deband]" in msg and words in msg, (what, msg)
    assert call(db, s, t, 0)[0] == 1                                    # nothing to filter: 1
    with pytest.raises(AmtError):
        db.run(src, cut(dst, 0, 2))                                     # more frames than dst holds
    torch.cuda.synchronize()
    for g, a in zip(download(dst_host, dst_flat), dst_host.flat):
        assert np.array_equal(g, a)                                     # still the sentinel, everywhere

    # set_offsets: one entry beyond lim, in the middle and on the rim; the table stays as it was
    before = db.offsets(0)
    lim = R.lim_map(w, h, radius)
    for (y, x), which, sign in (((10, 17), 0, 1), ((10, 17), 1, -1), ((0, 5), 0, 1), ((h - 1, w - 1), 1, -1), ((3, 20), 0, -1)):
        tabs = [np.zeros((h, w), np.int8), np.zeros((h, w), np.int8)]
        tabs[which][y, x] = sign * (lim[y, x] + 1)
        r = lib.amtgpu_deband_set_offsets(db.h, 0, tabs[0].ctypes.data_as(C.c_void_p), tabs[1].ctypes.data_as(C.c_void_p))
        assert r == 0 and "[Deband]" in last() and "lim" in last(), ((y, x), last())
    zeros = np.zeros((h // 2, w // 2), np.int8)
    for plane in (-1, 3):
        assert lib.amtgpu_deband_set_offsets(db.h, plane, zeros.ctypes.data_as(C.c_void_p), zeros.ctypes.data_as(C.c_void_p)) == 0 and "[Deband]" in last()
        assert lib.amtgpu_deband_get_offsets(db.h, plane, None, None) == 0 and "[Deband]" in last()
    assert lib.amtgpu_deband_set_offsets(db.h, 1, None, zeros.ctypes.data_as(C.c_void_p)) == 0 and "[Deband]" in last()
    with pytest.raises(AmtError):
        db.set_offsets(1, np.zeros((h, w), np.int8), np.zeros((h, w), np.int8))            # the luma plane's shape for a chroma plane
    with pytest.raises(AmtError, match="lim"):
        db.set_offsets(2, np.full((h // 2, w // 2), 1, np.int8), zeros)
    after = db.offsets(0)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # ... and after all of it the object filters as it was made to
    assert call(db, s, t, N)[0] == 1
    torch.cuda.synchronize()
    check_against("after the refusals", dst_host, download(dst_host, dst_flat), R.filter_clip(planes, bits, radius, 32767, 2, True))
    for g, a in zip(download(src_host, src_flat), src_host.flat):
        assert np.array_equal(g, a)
    db.close()
    db10.close()
