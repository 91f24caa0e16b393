"""The cadence renderer's edge-directed, motion-adaptive bob on the GPU (amtgpu_kfm_render_deint with AMTGPU_DEINT_ADAPTIVE; DESIGN.md
section 6d) against its numpy restatement (tests/kfm_render_adaptive_ref.py): every destination byte of the three planes, row padding and
the gaps between frames included, on both kernel forms and three depths, with rows longer than one round of a wave, tails, planes
narrower than one lane, a planted diagonal with a literal known answer across a lane boundary and across the seam between rounds, planted
extremes, a clip cut into batches, the line rule through the new entry point, and every new refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import kfm_render_adaptive_ref as A
import kfm_render_ref as R
import test_gpu_kfm_render as G
import test_gpu_kfm_render_surfaces as GS
from test_gpu_kfm_render import gpu  # noqa: F401  (the module's context fixture)

pytestmark = pytest.mark.gpu

W_, T_, B_ = R.WEAVE, R.BOB_TOP, R.BOB_BOTTOM
LINE, ADAPTIVE = 0, 1

# name: (width, height, bits, pitchY, pitchUV, gapY, gapUV)   pitches and the gap behind a frame's last row in containers
SHAPES = {
    "96x36-8-aligned": (96, 36, 8, 96, 48, 0, 0),               # the vector form, three depths
    "96x36-10-aligned": (96, 36, 10, 96, 48, 0, 0),
    "96x36-16-aligned": (96, 36, 16, 96, 48, 0, 0),
    "90x38-8-tail": (90, 38, 8, 96, 48, 0, 0),                  # a tail whose left neighbours sit in the vector part; chroma width 45 and
    "90x38-10-tail": (90, 38, 10, 96, 48, 0, 0),                # 19 chroma rows: the last row has no row below and none two below
    "90x38-8-element": (90, 38, 8, 91, 46, 3, 1),               # the element form
    "90x38-16-element": (90, 38, 16, 91, 46, 1, 1),
    "1100x8-8-long-rows": (1100, 8, 8, 1104, 560, 0, 0),        # a row longer than one round of the wave: a neighbour across the seam
    "530x8-16-long-rows": (530, 8, 16, 536, 272, 0, 0),
    "34x6-8-tail-34": (34, 6, 8, 48, 32, 0, 0),                 # two full lanes and a 2-byte tail
    "6x4-8-tiny-vector": (6, 4, 8, 16, 16, 0, 0),               # chroma 3x2: every column clamp and every row clamp at once, rows shorter
    "6x4-8-tiny-element": (6, 4, 8, 7, 5, 1, 1),                # than one lane; once with pitches that are multiples of 16 bytes, once not
    "6x4-16-tiny-vector": (6, 4, 16, 8, 8, 0, 0),
    "6x4-16-tiny-element": (6, 4, 16, 7, 5, 1, 1),
}
NSRC = 6
# both bobs at frame 0, at the last frame and mid-clip (2: the planted frame, and 3); WEAVE with top != bottom in both orders and a plain one
PLAN = R.plan_array([(T_, 0, 0, 1), (B_, 0, 0, 1), (W_, 3, 2, 2), (T_, 2, 2, 1), (B_, 2, 2, 1), (W_, 1, 1, 2), (W_, 2, 3, 2), (T_, 5, 5, 1), (B_, 5, 5, 1),
                     (T_, 3, 3, 1), (B_, 3, 3, 1)])
OUT_T2, OUT_B2 = 3, 4                                            # the outputs that are BOB_TOP(2) and BOB_BOTTOM(2)
WEAVES = [i for i, e in enumerate(PLAN) if e["kind"] == W_]


def diagonal_columns(shape):
    """first columns of the planted 16x8 diagonal patches (luma rows 0..7, frames 1..3): the edge of row 3 (column x0 + 7) starts a
    16-byte lane, and in the long rows the one behind byte 1024 as well"""
    w, h, bits = shape[:3]
    if w < 25 or h < 8:
        return []
    es = 1 if bits <= 8 else 2
    return [9] + ([1024 // es - 7] if w * es > 1024 + 16 else [])


def plant(clip):
    shape = (clip.w, clip.h, clip.bits)
    Y = clip.planes[0]
    top = 255 if clip.bits <= 8 else 65535
    for x0 in diagonal_columns(shape):
        # the known answer of the issue: frame n: row y is 0 left of column 4 + y and 200 from there; frame n - 1 all 0, frame n + 1 all 255
        Y[1, 0:8, x0:x0 + 16] = 0
        Y[3, 0:8, x0:x0 + 16] = 255
        for y in range(8):
            Y[2, y, x0:x0 + 16] = np.where(np.arange(16) < 4 + y, 0, 200)
    if clip.w >= 34 and clip.h >= 6:
        # containers 0 and top as c / e / A / B / b / f of the pixels (row 3, columns 28..31) of BOB_TOP(2): c = F2[2], e = F2[4], A = F1[3],
        # B = F2[3], b from row 1 and f from row 5 of F1 and F2
        Y[2, 2, 28:32] = (top, 0, top, top); Y[2, 4, 28:32] = (0, top, top, top)
        Y[1, 3, 28:32] = (0, top, top, 0); Y[2, 3, 28:32] = (top, top, top, 0)
        Y[1, 1, 28:32] = (top, 0, top, top); Y[2, 1, 28:32] = (top, 0, top, top)
        Y[1, 5, 28:32] = (0, top, top, top); Y[2, 5, 28:32] = (0, top, top, top)
    if clip.bits == 10:
        Y[2, 10, 40] = 0xFFFF; Y[2, 12, 41] = 0x0401; Y[1, 11, 40] = 0xFC00; clip.planes[1][3, 5, 7] = 0x8000     # beyond 10 bits: taken as stored


@functools.lru_cache(maxsize=None)
def source_clip(name):
    clip = G.HostClip(NSRC, SHAPES[name], rng=np.random.default_rng(sum(map(ord, name)) * 11 + 5))
    plant(clip)
    for a in clip.flat:
        a.setflags(write=False)
    return clip


@functools.lru_cache(maxsize=None)
def reference(name):
    """((Y, U, V) of PLAN, the counts): computed once per shape and shared"""
    want, counts = A.render_adaptive_ref(source_clip(name).planes, PLAN)
    for p in want:
        p.setflags(write=False)
    return want, counts


def render(gpu, src, plan, dst, deint, thresh=-1, src_first=0, clip_frames=None):
    """(return value, message) of amtgpu_kfm_render_deint on DeviceSurfaces"""
    ctx, torch = gpu
    s, d = src.ref(), dst.ref()
    return raw_deint(ctx, s, src_first, src.num_frames, src_first + src.num_frames if clip_frames is None else clip_frames, src.width, src.height, plan, deint, thresh, d)


def raw_deint(ctx, s, src_first, nsrc, clip_frames, w, h, plan, deint, thresh, d):
    pl = np.ascontiguousarray(plan, R.RENDER_FRAME).reshape(-1)
    r = ctx.lib.amtgpu_kfm_render_deint(ctx.h, C.byref(s), src_first, nsrc, clip_frames, w, h, pl.ctypes.data_as(C.c_void_p), len(pl), deint, thresh, C.byref(d))
    return r, ctx.lib.amtgpu_last_error(ctx.h).decode(errors="replace")


def assert_buffers(got, want, *what):
    for k, (g, e) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, (*what, "plane", k, "first differing element", int(bad[0]), int(g[bad[0]]), int(e[bad[0]]))


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_plane_byte_matches_the_reference(gpu, name):
    from amatsukaze_amd import kfm_render
    ctx, torch = gpu
    shape = SHAPES[name]
    clip = source_clip(name)
    want, counts = reference(name)
    Yw = want[0].astype(np.int64)
    # the planted diagonal is the literal known answer, where the rule sees nothing but the patch (3 columns inside it)
    cols = diagonal_columns(shape)
    assert cols or shape[0] < 25 or shape[1] < 8
    for x0 in cols:
        assert list(Yw[OUT_T2, 3, x0 + 3:x0 + 13]) == [0] * 4 + [200] * 6                  # 0 for x < 7, 200 from x = 7: the exact diagonal
        assert list(Yw[OUT_B2, 4, x0 + 3:x0 + 13]) == [0] * 5 + [200] * 5                  # 0 for x < 8, 200 from x = 8
        line = R.render_ref(clip.planes, PLAN[OUT_T2:OUT_T2 + 1], -1)[0].astype(np.int64)
        assert list(line[0, 3, x0 + 6:x0 + 8]) == [100, 100]                               # the line rule's staircase
    if "tiny" not in name:
        # so that a later change of seed cannot hollow the test out
        assert all(c > 0 for c in counts[0]["dir"]), (name, counts[0])
        assert all(c > 0 for c in counts[0]["clamp"]), (name, counts[0])

    src, src_flat = G.upload(gpu, clip)
    dst_host = G.sentinel_clip(len(PLAN), shape)
    dst, dst_flat = G.upload(gpu, dst_host)
    kfm_render(ctx, src, PLAN, dst, deint="adaptive")
    torch.cuda.synchronize()
    assert_buffers(G.download(dst_host, dst_flat), G.expected_buffers(dst_host, want), name)
    for g, a in zip(G.download(clip, src_flat), clip.flat):
        assert np.array_equal(g, a)                                                          # the sources are unchanged


@pytest.mark.parametrize("name", ["96x36-8-aligned", "90x38-16-element"])
def test_weave_frames_of_an_adaptive_call_are_those_of_a_line_call(gpu, name):
    ctx, torch = gpu
    clip = source_clip(name)
    src, _ = G.upload(gpu, clip)
    dst_host = G.sentinel_clip(len(PLAN), SHAPES[name])
    got = []
    for deint in (ADAPTIVE, LINE):
        dst, dst_flat = G.upload(gpu, dst_host)
        assert render(gpu, src, PLAN, dst, deint)[0] == 1
        torch.cuda.synchronize()
        got.append(G.download(dst_host, dst_flat))
    for k in range(3):
        a, l = dst_host.view(k, got[0][k]), dst_host.view(k, got[1][k])
        assert np.array_equal(a[WEAVES], l[WEAVES])
        assert not np.array_equal(a[OUT_T2], l[OUT_T2])                                      # and the bobs are not


@pytest.mark.parametrize("thresh", [-1, 0, 3])
def test_the_line_rule_through_the_new_entry_point_is_kfm_render_on_planes(gpu, thresh):
    ctx, torch = gpu
    name = "90x38-8-tail"
    clip = source_clip(name)
    src, _ = G.upload(gpu, clip)
    dst_host = G.sentinel_clip(len(PLAN), SHAPES[name])
    old, old_flat = G.upload(gpu, dst_host)
    new, new_flat = G.upload(gpu, dst_host)
    assert G.raw_render(ctx, src.ref(), 0, NSRC, NSRC, clip.w, clip.h, PLAN, thresh, old.ref())[0] == 1
    assert render(gpu, src, PLAN, new, LINE, thresh)[0] == 1
    torch.cuda.synchronize()
    one, two = G.download(dst_host, old_flat), G.download(dst_host, new_flat)
    assert_buffers(two, one, thresh)
    assert_buffers(one, G.expected_buffers(dst_host, R.render_ref(clip.planes, PLAN, thresh)), thresh)


@pytest.mark.parametrize("thresh", [-1, 0, 3])
def test_the_line_rule_through_the_new_entry_point_is_kfm_render_on_nv12(gpu, thresh):
    ctx, torch = gpu
    shape = GS.SHAPES["nv12-90x38-tail"]
    c = GS.Surf(NSRC, shape, rng=np.random.default_rng(77))
    src, _ = GS.upload(gpu, c)
    dst_host = GS.sentinel_surf(len(PLAN), shape)
    old, old_flat = GS.upload(gpu, dst_host)
    new, new_flat = GS.upload(gpu, dst_host)
    assert G.raw_render(ctx, src.ref(), 0, NSRC, NSRC, c.w, c.h, PLAN, thresh, old.ref())[0] == 1
    assert render(gpu, src, PLAN, new, LINE, thresh)[0] == 1
    torch.cuda.synchronize()
    one, two = GS.download(dst_host, old_flat), GS.download(dst_host, new_flat)
    assert_buffers(two, one, thresh)
    assert any((a != b).any() for a, b in zip(one, dst_host.flat))                           # something was rendered


def test_a_clip_cut_into_batches_gives_the_bytes_of_one_call(gpu):
    from amatsukaze_amd import DeviceSurfaces, kfm_render
    ctx, torch = gpu
    name = "90x38-8-tail"
    shape = SHAPES[name]
    clip = source_clip(name)
    plan = R.plan_array([e for n in range(NSRC) for e in ((T_, n, n, 1), (B_, n, n, 1))])
    want, _ = A.render_adaptive_ref(clip.planes, plan)
    src, _ = G.upload(gpu, clip)
    dst_host = G.sentinel_clip(len(plan), shape)
    whole, whole_flat = G.upload(gpu, dst_host)
    kfm_render(ctx, src, plan, whole, deint="adaptive")
    # 2 + 2 + 2: the batch that owns frames [lo, hi) carries one frame on either side as its halo
    parts, parts_flat = G.upload(gpu, dst_host)
    cut = lambda s, i, j: DeviceSurfaces(s.Y[i:j], s.U[i:j], s.V[i:j], s.width, s.height, s.bits)
    for lo, hi in ((0, 2), (2, 4), (4, 6)):
        a, b = max(0, lo - 1), min(NSRC, hi + 1)
        kfm_render(ctx, cut(src, a, b), plan[2 * lo:2 * hi], cut(parts, 2 * lo, 2 * hi), src_first=a, clip_frames=NSRC, deint="adaptive")
    torch.cuda.synchronize()
    one, three = G.download(dst_host, whole_flat), G.download(dst_host, parts_flat)
    e = G.expected_buffers(dst_host, want)
    assert_buffers(one, e, "one call")
    assert_buffers(three, e, "three calls")


def test_new_refusals_launch_nothing(gpu):
    from amatsukaze_amd import AmtError, DeviceSurfaces, binding, kfm_render
    ctx, torch = gpu
    name = "96x36-8-aligned"
    shape = SHAPES[name]
    W, H, N = 96, 36, NSRC
    clip = source_clip(name)
    src, src_flat = G.upload(gpu, clip)
    dst_host = G.sentinel_clip(4, shape)
    dst, dst_flat = G.upload(gpu, dst_host)
    s, d = src.ref(), dst.ref()
    plan = lambda *e: R.plan_array(list(e))
    ok = plan((T_, 2, 2, 1))

    def changed(desc, **kw):
        c = binding.Surfaces()
        C.memmove(C.byref(c), C.byref(desc), C.sizeof(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    mid = DeviceSurfaces(src.Y[2:5], src.U[2:5], src.V[2:5], W, H, 8).ref()                # frames 2..4 of a clip of 8
    s10, d10 = changed(s, bits=10, pitchY=48, pitchUV=24), changed(d, bits=10, pitchY=48, pitchUV=24)
    cases = {
        # name: (arguments, a word the message must hold)
        "thresh 0": ((s, 0, N, N, W, H, ok, ADAPTIVE, 0, d), "thresh"),
        "thresh 4": ((s, 0, N, N, W, H, ok, ADAPTIVE, 4, d), "thresh"),
        "thresh -2": ((s, 0, N, N, W, H, ok, ADAPTIVE, -2, d), "thresh"),
        "deint 2": ((s, 0, N, N, W, H, ok, 2, -1, d), "deint"),
        "deint -1": ((s, 0, N, N, W, H, ok, -1, -1, d), "deint"),
        "BOB_TOP without frame n - 1": ((mid, 2, 3, 8, W, H, plan((W_, 3, 3, 2), (T_, 2, 2, 1)), ADAPTIVE, -1, d), "plan entry 1: the neighbour frame 1 "),
        "BOB_TOP without frame n + 1": ((mid, 2, 3, 8, W, H, plan((T_, 4, 4, 1)), ADAPTIVE, -1, d), "plan entry 0: the neighbour frame 5 "),
        "BOB_BOTTOM without frame n - 1": ((mid, 2, 3, 8, W, H, plan((B_, 2, 2, 1)), ADAPTIVE, -1, d), "plan entry 0: the neighbour frame 1 "),
        "BOB_BOTTOM without frame n + 1": ((mid, 2, 3, 8, W, H, plan((B_, 4, 4, 1)), ADAPTIVE, -1, d), "plan entry 0: the neighbour frame 5 "),
        "NV12 pair": ((changed(s, interleaved=1, pitchUV=96), 0, N, N, W, H, ok, ADAPTIVE, -1, changed(d, interleaved=1, pitchUV=96)), "planes only"),
        "planar MSB pair": ((changed(s10, msb_aligned=1), 0, N, N, W // 2, H, ok, ADAPTIVE, -1, changed(d10, msb_aligned=1)), "planes only"),
        "P010 pair": ((changed(s10, msb_aligned=1, interleaved=1, pitchUV=48), 0, N, N, W // 2, H, ok, ADAPTIVE, -1,
                      changed(d10, msb_aligned=1, interleaved=1, pitchUV=48)), "planes only"),
        # and those of the existing call
        "odd width": ((s, 0, N, N, W - 1, H, ok, ADAPTIVE, -1, d), ""),
        "kind 3": ((s, 0, N, N, W, H, plan((3, 0, 0, 2)), ADAPTIVE, -1, d), ""),
        "BOB_TOP with top != bottom": ((s, 0, N, N, W, H, plan((T_, 1, 2, 1)), ADAPTIVE, -1, d), ""),
        "top behind the batch": ((s, 0, N, N, W, H, plan((W_, N, 0, 2)), ADAPTIVE, -1, d), ""),
        "destination is the source": ((s, 0, N, N, W, H, ok, ADAPTIVE, -1, s), ""),
        "NV12 source, planar destination": ((changed(s, interleaved=1), 0, N, N, W, H, ok, ADAPTIVE, -1, d), ""),
        "different depths": ((s, 0, N, N, W, H, ok, ADAPTIVE, -1, changed(d, bits=10)), ""),
    }
    for what, (args, word) in cases.items():
        r, msg = raw_deint(ctx, *args)
        assert r == 0 and msg.strip() and word in msg, (what, msg)
    with pytest.raises(AmtError, match="thresh"):
        kfm_render(ctx, src, ok, dst, thresh=3, deint="adaptive")
    with pytest.raises(AmtError, match="deint"):
        kfm_render(ctx, src, ok, dst, deint="yadif")
    torch.cuda.synchronize()
    for g, a in zip(G.download(dst_host, dst_flat), dst_host.flat):
        assert np.array_equal(g, a)                                                          # still the sentinel, everywhere
    for g, a in zip(G.download(clip, src_flat), clip.flat):
        assert np.array_equal(g, a)
    # at the clip's ends there are no neighbours to need: a clip of one frame renders
    ends = DeviceSurfaces(src.Y[0:1], src.U[0:1], src.V[0:1], W, H, 8).ref()
    both = plan((T_, 0, 0, 1), (B_, 0, 0, 1))
    assert raw_deint(ctx, ends, 0, 1, 1, W, H, both, ADAPTIVE, -1, d)[0] == 1
    torch.cuda.synchronize()
    want, _ = A.render_adaptive_ref(tuple(p[0:1] for p in clip.planes), both)
    got = G.download(dst_host, dst_flat)
    for k in range(3):
        assert np.array_equal(dst_host.view(k, got[k])[:2, :, :dst_host.geom[k][1]], want[k])
