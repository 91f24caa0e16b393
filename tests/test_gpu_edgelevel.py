"""The edge level on the GPU (amtgpu_edgelevel) against its numpy restatement (tests/edgelevel_ref.py, which
tests/test_edgelevel_host.py holds against the rule's known answers): every destination container of the three planes, guard containers
behind the rows and around the frames included, on both kernel forms and both container sizes; planes that are all border, an interior
of 2 x 2, a wave's seam with a second span and a tail that is no whole lane, a strip's seam with its halo rows and a short last strip;
the server's parameters, every repair, the ends of strength and threshold; planted pixels on every boundary of the rule at lane 0, lane
63, in a row's last span and in the first and last row of a strip; a clip cut into calls; and every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import edgelevel_ref as R
from test_gpu_deband import aligned_layouts
from test_gpu_temporal_nr import Buf, check_against, cut, download, narrow_layouts, sentinel_buf, upload

pytestmark = pytest.mark.gpu

# mirrored from csrc/kernels.hpp (tests/test_edgelevel_host.py holds the lines against the file)
STRIP, SPAN_BYTES = 32, 64 * 16
# (bits, bits of the content): 8-bit containers; 16-bit containers with 14-bit and with full 16-bit content
DEPTHS = [(8, 8), (14, 14), (16, 16)]
LAYOUTS = {"aligned": aligned_layouts, "one-off": narrow_layouts}
# the server's; every repair; strength 0 and 255; threshold 0 and 32767
PARAMS = [(16, 10, 2), (16, 10, 0), (16, 10, 1), (16, 10, 3), (16, 10, 4), (0, 10, 2), (255, 10, 2), (16, 0, 2), (255, 0, 0), (16, 32767, 2)]


def es_of(bits):
    return 1 if bits <= 8 else 2


def sizes(bits):
    """all border; an interior of 2 x 2; one lane and a tail; a wave's span plus 34 containers; two strips plus 6 rows"""
    span = SPAN_BYTES // es_of(bits)
    return [(4, 4), (6, 6), (40, 12), (span + 34, 12), (40, 2 * STRIP + 6)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    ctx = Context(0)
    yield ctx, torch
    ctx.close()


def run_case(gpu, what, planes, bits, layouts, want, params):
    """one call over the whole clip: every destination container against `want`, the sources unchanged"""
    from amatsukaze_amd import edge_level
    ctx, torch = gpu
    n, h, w = planes[0].shape
    sl, dl = layouts(w, h, bits)
    src_host = Buf(n, w, h, bits, **sl).put(planes)
    dst_host = sentinel_buf(n, w, h, bits, dl)
    src, src_flat = upload(gpu, src_host)
    dst, dst_flat = upload(gpu, dst_host)
    assert edge_level(ctx, src, dst, *params) == n
    torch.cuda.synchronize()
    check_against(what, dst_host, download(dst_host, dst_flat), want)
    for g, a in zip(download(src_host, src_flat), src_host.flat):
        assert np.array_equal(g, a), (what, "the source changed")


# ---- every size, depth and lane form; under each every parameter set on both contents ----
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("depth", DEPTHS, ids=lambda d: "bits%d-content%d" % d)
@pytest.mark.parametrize("size", range(5), ids=["all-border", "interior-2x2", "one-lane", "wave-seam", "strip-seam"])
def test_every_size_depth_form_and_parameter(gpu, size, depth, layout):
    bits = depth[0]
    w, h = sizes(bits)[size]
    for kind in ("random", "soft"):
        planes = R.clip(w, h, depth, kind)
        changed = 0
        for params in PARAMS:
            want = R.filter_clip(planes, bits, *params)
            changed += int(not np.array_equal(want[0], planes[0]))
            run_case(gpu, ((w, h), depth, layout, kind, params), planes, bits, LAYOUTS[layout], want, params)
        # the cases were worth running: a plane without an interior is copied; one with a real interior is changed by every parameter set
        # but threshold 32767, which never does, and at most one more (strength 0 leaves the change to the repair)
        if h < 5:
            assert changed == 0, (kind, changed)
        elif w >= 40:
            assert len(PARAMS) - 2 <= changed < len(PARAMS), (kind, changed)


# ---- planted pixels on the rule's boundaries, at the kernel's seams ----
@functools.lru_cache(maxsize=None)
def planted_clip(depth):
    """one frame per (line of edgelevel_ref.boundary_lines, orientation, group of columns, group of rows): a constant plane with the line's
    centre at every (row, column) of the two groups.  Returns (planes, [(frame, y, x, vertical, changes)])"""
    bits, content = depth
    span, px = SPAN_BYTES // es_of(bits), 16 // es_of(bits)
    w, h = span + 34, 2 * STRIP + 6
    dt = np.uint8 if bits <= 8 else np.uint16
    # columns: the first interior one (lane 0), a lane's last and the next lane's first, lane 63's last and the second span's first
    # (the wave's seam), the last interior one (the row's last span, in its tail).  Rows: the first interior one, the last of a
    # strip and the first of the next, twice, and the last interior one.  Neighbours are kept in different groups: no two lines touch
    col_groups = ([2, px - 1, span - 1, w - 3], [px, span])
    row_groups = ([2, STRIP - 1, 2 * STRIP - 1], [STRIP, 2 * STRIP], [h - 3])
    frames, where = [], []
    for name, (line, changes) in R.boundary_lines(bits).items():
        for vertical in (False, True):
            for cols in col_groups:
                for rows in row_groups:
                    s = np.full((h, w), line[2], dt)
                    for y in rows:
                        for x in cols:
                            if vertical:
                                s[y - 2:y + 3, x] = line
                            else:
                                s[y, x - 2:x + 3] = line
                            where.append((len(frames), y, x, vertical, changes))
                    frames.append(s)
    Y = np.stack(frames)
    rng = np.random.default_rng(content)
    U, V = (rng.integers(0, 1 << content, (len(frames), h // 2, w // 2)).astype(dt) for _ in range(2))
    for p in (Y, U, V):
        p.setflags(write=False)
    return (Y, U, V), where


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("depth", DEPTHS, ids=lambda d: "bits%d-content%d" % d)
def test_planted_boundary_pixels_at_the_seams(gpu, depth, layout):
    bits = depth[0]
    planes, where = planted_clip(depth)
    want0 = R.filter_clip(planes, bits, 16, 10, 0)
    for f, y, x, vertical, changes in where:
        # the planted pixel is what the host test planted: on its boundary it stays, one beyond it moves
        assert (want0[0][f, y, x] != planes[0][f, y, x]) == changes, (f, y, x, vertical)
    run_case(gpu, (depth, layout, "planted", 0), planes, bits, LAYOUTS[layout], want0, (16, 10, 0))
    run_case(gpu, (depth, layout, "planted", 2), planes, bits, LAYOUTS[layout], R.filter_clip(planes, bits, 16, 10, 2), (16, 10, 2))


# ---- a clip cut into calls ----
@pytest.mark.parametrize("bits", [8, 14])
def test_calls_of_2_and_3_frames_give_the_bytes_of_one_call(gpu, bits):
    from amatsukaze_amd import edge_level
    ctx, torch = gpu
    w, h, N = SPAN_BYTES // es_of(bits) + 34, 12, 5
    planes = R.clip(w, h, (bits, bits), "soft", N)
    want = R.filter_clip(planes, bits)                                  # the defaults: 16, 10, 2
    sl, dl = aligned_layouts(w, h, bits)
    src, _ = upload(gpu, Buf(N, w, h, bits, **sl).put(planes))
    dst_host = sentinel_buf(N, w, h, bits, dl)
    whole, whole_flat = upload(gpu, dst_host)
    parts, parts_flat = upload(gpu, dst_host)
    assert edge_level(ctx, src, whole) == N
    assert edge_level(ctx, cut(src, 0, 2), cut(parts, 0, 2)) == 2 and edge_level(ctx, cut(src, 2, 5), cut(parts, 2, 5)) == 3
    torch.cuda.synchronize()
    one, many = download(dst_host, whole_flat), download(dst_host, parts_flat)
    check_against("one call", dst_host, one, want)
    assert all(not np.array_equal(want[0][f], planes[0][f]) for f in range(N))
    for g1, g2 in zip(one, many):
        assert np.array_equal(g1, g2)


# ---- refusals ----
def test_refusals_write_nothing(gpu):
    from amatsukaze_amd import AmtError, binding, edge_level
    ctx, torch = gpu
    N, w, h, bits = 3, 34, 20, 8
    planes = R.clip(w, h, (8, 8), "random", N)
    sl, dl = aligned_layouts(w, h, bits)
    src_host = Buf(N, w, h, bits, **sl).put(planes)
    src, src_flat = upload(gpu, src_host)
    dst_host = sentinel_buf(N, w, h, bits, dl)
    dst, dst_flat = upload(gpu, dst_host)
    s, t = src.ref(), dst.ref()
    lib = ctx.lib
    last = lambda: lib.amtgpu_last_error(ctx.h).decode(errors="replace")

    def changed(desc, **kw):
        c = binding.Surfaces()
        C.memmove(C.byref(c), C.byref(desc), C.sizeof(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def call(s_, t_, n=N, width=w, height=h, strength=16, threshold=10, repair=2):
        r = lib.amtgpu_edgelevel(ctx.h, None if s_ is None else C.byref(s_), None if t_ is None else C.byref(t_), width, height, n, strength, threshold, repair)
        return r, last()

    cases = {
        # name: (arguments, keywords, words the message must hold)
        "null source": ((None, t), {}, "null surface descriptor"),
        "null destination": ((s, None), {}, "null surface descriptor"),
        "odd width": ((s, t), dict(width=w - 1), "width and height must be even and positive"),
        "odd height": ((s, t), dict(height=h - 1), "width and height must be even and positive"),
        "no width": ((s, t), dict(width=0), "width and height must be even and positive"),
        "negative height": ((s, t), dict(height=-2), "width and height must be even and positive"),
        "bits 7": ((changed(s, bits=7), changed(t, bits=7)), {}, "surface bits must be 8..16"),
        "bits 17": ((s, changed(t, bits=17)), {}, "surface bits must be 8..16"),
        "sides of other bits": ((changed(s, bits=10), changed(t, bits=12)), {}, "source and destination differ in bits"),
        "negative frame count": ((s, t), dict(n=-1), "negative frame count"),
        "strength -1": ((s, t), dict(strength=-1), "strength must be 0..255"),
        "strength 256": ((s, t), dict(strength=256), "strength must be 0..255"),
        "threshold -1": ((s, t), dict(threshold=-1), "threshold must be 0..32767"),
        "threshold 32768": ((s, t), dict(threshold=32768), "threshold must be 0..32767"),
        "repair -1": ((s, t), dict(repair=-1), "repair must be 0..4"),
        "repair 5": ((s, t), dict(repair=5), "repair must be 0..4"),
        "interleaved source": ((changed(s, interleaved=1), t), {}, "source: planar, LSB-aligned planes only"),
        "interleaved destination": ((s, changed(t, interleaved=1)), {}, "destination: planar, LSB-aligned planes only"),
        "MSB-aligned source": ((changed(s, bits=10, msb_aligned=1), changed(t, bits=10)), {}, "source: planar, LSB-aligned planes only"),
        "MSB-aligned destination": ((changed(s, bits=10), changed(t, bits=10, msb_aligned=1)), {}, "destination: planar, LSB-aligned planes only"),
        "source pitch below the row": ((changed(s, pitchY=w - 2), t), {}, "source: pitch smaller than the row"),
        "destination chroma pitch below the row": ((s, changed(t, pitchUV=w // 2 - 1)), {}, "destination: pitch smaller than the row"),
        "negative source stride": ((changed(s, strideY=-s.strideY), t), {}, "source: negative frame stride"),
        "negative destination chroma stride": ((s, changed(t, strideUV=-t.strideUV)), {}, "destination: negative frame stride"),
        "overlapping destination frames": ((s, changed(t, strideY=(h - 1) * t.pitchY + w - 1)), dict(n=2), "destination frames overlap each other"),
        "destination is the source": ((s, s), {}, "overlaps the source's"),
        "destination luma inside the source's chroma": ((s, changed(t, Y=s.U)), dict(n=1), "overlaps the source's"),
        "destination one byte into the source": ((s, changed(t, V=s.Y + s.strideY * (N - 1) + (h - 1) * s.pitchY + w - 1)), {}, "overlaps the source's"),
        "pitch above 2 GiB": ((changed(s, bits=16, pitchY=1 << 30), changed(t, bits=16)), dict(n=1), "pitch above 2 GiB"),
        "null source plane": ((changed(s, V=None), t), {}, "null surface plane"),
    }
    for what, (args, kw, words) in cases.items():
        r, msg = call(*args, **kw)
        assert r == 0 and "[EdgeLevel]" in msg and words in msg, (what, msg)
    assert "no in-place filtering" in call(s, s)[1]
    assert call(s, t, n=0)[0] == 1                                       # nothing to filter: 1
    with pytest.raises(AmtError, match="EdgeLevel"):
        edge_level(ctx, src, dst, repair=5)
    with pytest.raises(AmtError):
        edge_level(ctx, src, cut(dst, 0, 2))                            # more frames than dst holds
    torch.cuda.synchronize()
    for g, a in zip(download(dst_host, dst_flat), dst_host.flat):
        assert np.array_equal(g, a)                                     # still the sentinel, everywhere
    # ... and after all of it the call filters
    assert call(s, t)[0] == 1
    torch.cuda.synchronize()
    check_against("after the refusals", dst_host, download(dst_host, dst_flat), R.filter_clip(planes, bits))
    for g, a in zip(download(src_host, src_flat), src_host.flat):
        assert np.array_equal(g, a)
