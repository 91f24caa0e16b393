"""The adaptive bob on decoder surfaces on the GPU (amtgpu_kfm_render_deint_surfaces with AMTGPU_DEINT_ADAPTIVE on NV12 / P010 / P012 /
P016 / interleaved LSB / planar MSB pairs in kind) against its composed numpy restatement
(tests/kfm_render_adaptive_surfaces_ref.py): every destination byte, row padding and the gaps between frames included, on all eight
kernel forms, with UV rows longer than one round of a wave, tails, a UV row of exactly one lane, rows shorter than a lane, planted
diagonals with a literal known answer in luma and in chroma across a lane boundary and across the seam between rounds, planted extremes,
random low bits, a clip cut into batches, the line rule and planar pairs through the new entry point, the route over weave_fields that
was the only one before, and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import kfm_render_adaptive_surfaces_ref as AS
import kfm_render_ref as R
import kfm_render_surfaces_ref as S
import test_gpu_kfm_render as G
import test_gpu_kfm_render_adaptive as GA
import test_gpu_kfm_render_surfaces as GS
from test_gpu_kfm_render import gpu  # noqa: F401  (the module's context fixture)
from test_gpu_kfm_render_adaptive import ADAPTIVE, LINE, NSRC, OUT_B2, OUT_T2, PLAN
from test_gpu_kfm_render_surfaces import Surf, download, expected_buffers, sentinel_surf, upload

pytestmark = pytest.mark.gpu

W_, T_, B_ = R.WEAVE, R.BOB_TOP, R.BOB_BOTTOM

# name: (width, height, bits, interleaved, msb, pitchY, pitchUV, gapY, gapUV, one_allocation), as test_gpu_kfm_render_surfaces.SHAPES
SHAPES = {
    "nv12-96x36-aligned": GS.SHAPES["nv12-96x36-aligned"],                        # the vector forms
    "nv12-90x38-tail": GS.SHAPES["nv12-90x38-tail"],                              # ... with a tail
    "nv12-90x38-element": GS.SHAPES["nv12-90x38-element"],                        # the element form (pitch 91, gaps)
    "nv12-1100x8-long-rows": GS.SHAPES["nv12-1100x8-long-rows"],                  # a UV row over 1 024 bytes: a step-2 neighbour across the seam
    "nv12-96x36-one-allocation": GS.SHAPES["nv12-96x36-one-allocation"],          # Y and UV of a frame behind each other
    "nv12-34x8": (34, 8, 8, True, False, 48, 48, 0, 0, False),                    # two full lanes and a 2-byte tail in the UV row
    "nv12-16x8-one-lane": (16, 8, 8, True, False, 16, 16, 0, 0, False),           # a UV row of exactly one 16-byte span: one lane that is first
    "p010-8x8-one-lane": (8, 8, 10, True, True, 8, 8, 0, 0, False),               # and last
    "nv12-6x8-pitch-16": (6, 8, 8, True, False, 16, 16, 0, 0, False),             # rows shorter than a lane, every column clamp: once with
    "nv12-6x8-odd-pitch": (6, 8, 8, True, False, 7, 7, 1, 1, False),              # pitches that are multiples of 16 bytes, once not
    "p010-6x8-pitch-16": (6, 8, 10, True, True, 8, 8, 0, 0, False),
    "p010-6x8-odd-pitch": (6, 8, 10, True, True, 7, 7, 1, 1, False),
    "nv12-6x4": (6, 4, 8, True, False, 16, 16, 0, 0, False),                      # chroma 3x2: every row clamp
    "p010-96x36-aligned": GS.SHAPES["p010-96x36-aligned"],                        # the MSB vector forms
    "p010-90x38-tail": GS.SHAPES["p010-90x38-tail"],
    "p010-90x38-element": GS.SHAPES["p010-90x38-element"],                        # the MSB element form
    "p010-530x8-long-rows": GS.SHAPES["p010-530x8-long-rows"],                    # an MSB row longer than one round of the wave
    "p012-96x36": GS.SHAPES["p012-96x36"],
    "p016-96x36-msb-flag-without-shift": GS.SHAPES["p016-96x36-msb-flag-without-shift"],
    "interleaved-lsb-10-90x38": GS.SHAPES["interleaved-lsb-10-90x38"],
    "planar-msb-10-90x38": GS.SHAPES["planar-msb-10-90x38"],
}


def luma_columns(c):
    """first columns of the planted luma diagonals, as test_gpu_kfm_render_adaptive.diagonal_columns: the edge of row 3 (column x0 + 7)
    starts a 16-byte lane, and in the long rows the one behind byte 1 024 as well"""
    es = np.dtype(c.dt).itemsize
    if c.w < 25 or c.h < 8:
        return []
    return [9] + ([1024 // es - 7] if c.w * es > 1024 + 16 else [])


def chroma_columns(c):
    """first component columns of the planted chroma diagonals: the edge of row 3 (component column x0 + 7; byte (x0 + 7) * es of a planar
    row, 2 * (x0 + 7) * es of a UV row) starts a 16-byte lane, and in the long rows the one behind byte 1 024 as well"""
    es, wc = np.dtype(c.dt).itemsize, c.w // 2
    step = 2 if c.interleaved else 1
    if wc < 17:
        return []
    return [9 if wc >= 25 else 1] + ([1024 // (step * es) - 7] if wc * step * es > 1024 + 16 else [])


def components(c):
    """writable views of the clip's U and V components [n, h/2, w/2], whatever the layout"""
    if c.interleaved:
        UV = c.planes[1]
        return UV[:, :, 0::2], UV[:, :, 1::2]
    return c.planes[1], c.planes[2]


def plant(c, rng):
    """samples planted as containers sample << s with random low bits where there are any (frames 1..3; BOB_TOP(2) and BOB_BOTTOM(2) are
    outputs OUT_T2 and OUT_B2 of PLAN)"""
    s, top = c.s, c.top
    low = lambda shape: rng.integers(0, 1 << s, shape).astype(c.dt) if s else 0
    put = lambda P, idx, samples: P.__setitem__(idx, (np.asarray(samples, np.int64) << s).astype(c.dt) | low(np.shape(P[idx])))
    Y = c.planes[0]
    U, V = components(c)
    for P, cols in ((Y, luma_columns(c)), (U, chroma_columns(c))):
        rows = min(8, P.shape[1])
        for x0 in cols:
            # frame n: row y is 0 left of patch column 4 + y and 200 from there; frame n - 1 all 0, frame n + 1 all 255 (the depth's top)
            put(P, (1, slice(0, rows), slice(x0, x0 + 16)), np.zeros((rows, 16)))
            put(P, (3, slice(0, rows), slice(x0, x0 + 16)), np.full((rows, 16), min(255, top)))
            for y in range(rows):
                put(P, (2, y, slice(x0, x0 + 16)), np.where(np.arange(16) < 4 + y, 0, 200))
    for P in (Y, V):                                                                         # (U has the diagonals)
        if P.shape[2] >= 17 and P.shape[1] >= 6:
            # samples 0 and top as c / e / A / B / b / f of the pixels (row 3, the plane's last four columns but one) of BOB_TOP(2)
            x = slice(P.shape[2] - 5, P.shape[2] - 1)
            put(P, (2, 2, x), (top, 0, top, top)); put(P, (2, 4, x), (0, top, top, top))
            put(P, (1, 3, x), (0, top, top, 0)); put(P, (2, 3, x), (top, top, top, 0))
            put(P, (1, 1, x), (top, 0, top, top)); put(P, (2, 1, x), (top, 0, top, top))
            put(P, (1, 5, x), (0, top, top, top)); put(P, (2, 5, x), (0, top, top, top))


@functools.lru_cache(maxsize=None)
def source(name):
    seed = sum(map(ord, name)) * 13 + 7
    c = Surf(NSRC, SHAPES[name], rng=np.random.default_rng(seed))
    plant(c, np.random.default_rng(seed + 1))
    for a in c.flat:
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the destination's tight planes of PLAN, the counts per plane Y, U, V): computed once per shape and shared"""
    c = source(name)
    want, counts = AS.render_adaptive_surfaces_ref(c.planes, PLAN, c.bits, c.interleaved, c.msb)
    for p in want:
        p.setflags(write=False)
    return want, counts


def raw_deint_surfaces(ctx, s, src_first, nsrc, clip_frames, w, h, plan, deint, thresh, d):
    """(return value, message) of amtgpu_kfm_render_deint_surfaces"""
    pl = np.ascontiguousarray(plan, R.RENDER_FRAME).reshape(-1)
    r = ctx.lib.amtgpu_kfm_render_deint_surfaces(ctx.h, C.byref(s), src_first, nsrc, clip_frames, w, h, pl.ctypes.data_as(C.c_void_p), len(pl), deint, thresh, C.byref(d))
    return r, ctx.lib.amtgpu_last_error(ctx.h).decode(errors="replace")


def assert_buffers(got, want, *what):
    for k, (g, e) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, (*what, "buffer", k, "first differing element", int(bad[0]), int(g[bad[0]]), int(e[bad[0]]), "differing", int(bad.size))


def check_planted(name, c, want, counts):
    """the planted diagonals are the literal known answer on the reference's output, where the rule sees nothing but the patch (3 columns
    inside it) and the plane has the patch's eight rows"""
    s = c.s
    Yw = want[0].astype(np.int64) >> s
    Uw = S.split_planes(want, c.interleaved)[1].astype(np.int64) >> s
    assert luma_columns(c) or c.w < 25 or c.h < 8
    assert chroma_columns(c) or c.w < 34
    for P, cols in ((Yw, luma_columns(c)), (Uw, chroma_columns(c))):
        if P.shape[1] < 8:
            continue
        for x0 in cols:
            assert list(P[OUT_T2, 3, x0 + 3:x0 + 13]) == [0] * 4 + [200] * 6, (name, x0)
            assert list(P[OUT_B2, 4, x0 + 3:x0 + 13]) == [0] * 5 + [200] * 5, (name, x0)
    if c.w >= 34 and c.h >= 8:
        # so that a later change of seed cannot hollow the test out: every direction and every clamp outcome, in Y, in U and in V
        for k in range(3):
            assert all(n > 0 for n in counts[k]["dir"]) and all(n > 0 for n in counts[k]["clamp"]), (name, k, counts[k])


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_surface_byte_matches_the_reference(gpu, name):
    from amatsukaze_amd import kfm_render
    ctx, torch = gpu
    c = source(name)
    want, counts = reference(name)
    check_planted(name, c, want, counts)
    src, src_flat = upload(gpu, c)
    assert (src.V is None) == c.interleaved
    dst_host = sentinel_surf(len(PLAN), SHAPES[name])
    dst, dst_flat = upload(gpu, dst_host)
    kfm_render(ctx, src, PLAN, dst, deint="adaptive")
    torch.cuda.synchronize()
    assert_buffers(download(dst_host, dst_flat), expected_buffers(dst_host, want), name)
    for g, a in zip(download(c, src_flat), c.flat):
        assert np.array_equal(g, a)                                                          # the sources are unchanged


@pytest.mark.parametrize("name", ["nv12-90x38-tail", "p010-90x38-tail"])
def test_a_clip_cut_into_batches_gives_the_bytes_of_one_call(gpu, name):
    from amatsukaze_amd import kfm_render
    ctx, torch = gpu
    shape = SHAPES[name]
    c = source(name)
    plan = R.plan_array([e for n in range(NSRC) for e in ((T_, n, n, 1), (B_, n, n, 1))])
    want, _ = AS.render_adaptive_surfaces_ref(c.planes, plan, c.bits, c.interleaved, c.msb)
    src, _ = upload(gpu, c)
    dst_host = sentinel_surf(len(plan), shape)
    whole, whole_flat = upload(gpu, dst_host)
    kfm_render(ctx, src, plan, whole, deint="adaptive")
    # 2 + 2 + 2: the batch that owns frames [lo, hi) carries one frame on either side as its halo
    parts, parts_flat = upload(gpu, dst_host)
    for lo, hi in ((0, 2), (2, 4), (4, 6)):
        a, b = max(0, lo - 1), min(NSRC, hi + 1)
        kfm_render(ctx, GS.cut(src, a, b), plan[2 * lo:2 * hi], GS.cut(parts, 2 * lo, 2 * hi), src_first=a, clip_frames=NSRC, deint="adaptive")
    torch.cuda.synchronize()
    expect = expected_buffers(dst_host, want)
    assert_buffers(download(dst_host, whole_flat), expect, name, "one call")
    assert_buffers(download(dst_host, parts_flat), expect, name, "three calls")


@pytest.mark.parametrize("thresh", [-1, 0, 3])
@pytest.mark.parametrize("name", ["nv12-90x38-tail", "p010-90x38-tail"])
def test_the_line_rule_through_the_new_entry_point_is_kfm_render(gpu, name, thresh):
    ctx, torch = gpu
    c = source(name)
    src, _ = upload(gpu, c)
    dst_host = sentinel_surf(len(PLAN), SHAPES[name])
    old, old_flat = upload(gpu, dst_host)
    new, new_flat = upload(gpu, dst_host)
    assert G.raw_render(ctx, src.ref(), 0, NSRC, NSRC, c.w, c.h, PLAN, thresh, old.ref())[0] == 1
    r, msg = raw_deint_surfaces(ctx, src.ref(), 0, NSRC, NSRC, c.w, c.h, PLAN, LINE, thresh, new.ref())
    assert r == 1, msg
    torch.cuda.synchronize()
    one, two = download(dst_host, old_flat), download(dst_host, new_flat)
    assert_buffers(two, one, name, thresh)
    assert_buffers(one, expected_buffers(dst_host, S.render_surfaces_ref(c.planes, PLAN, thresh, c.bits, c.interleaved, c.msb)), name, thresh)


@pytest.mark.parametrize("name", ["90x38-8-tail", "90x38-16-element"])
def test_a_planar_lsb_pair_through_the_new_entry_point_is_kfm_render_deint(gpu, name):
    ctx, torch = gpu
    clip = GA.source_clip(name)
    src, _ = G.upload(gpu, clip)
    dst_host = G.sentinel_clip(len(PLAN), GA.SHAPES[name])
    old, old_flat = G.upload(gpu, dst_host)
    new, new_flat = G.upload(gpu, dst_host)
    assert GA.render(gpu, src, PLAN, old, ADAPTIVE)[0] == 1
    r, msg = raw_deint_surfaces(ctx, src.ref(), 0, NSRC, NSRC, clip.w, clip.h, PLAN, ADAPTIVE, -1, new.ref())
    assert r == 1, msg
    torch.cuda.synchronize()
    one, two = G.download(dst_host, old_flat), G.download(dst_host, new_flat)
    GA.assert_buffers(two, one, name)
    GA.assert_buffers(one, G.expected_buffers(dst_host, GA.reference(name)[0]), name)


def test_p010_render_is_the_planar_adaptive_render_of_the_woven_samples(gpu):
    """the only route before: weave_fields(nv12=True, msb=True) planarises whole frames, the planar adaptive kernel renders them"""
    from amatsukaze_amd import DeviceClip, kfm_render, weave_fields
    ctx, torch = gpu
    shape = (90, 36, 10, True, True, 96, 96, 0, 0, False)                                   # (the weave wants a height that is a multiple of 4)
    c = Surf(NSRC, shape, rng=np.random.default_rng(10))
    src, _ = upload(gpu, c)
    dst_host = sentinel_surf(len(PLAN), shape)
    dst, dst_flat = upload(gpu, dst_host)
    kfm_render(ctx, src, PLAN, dst, deint="adaptive")
    mk = lambda n, h, w: torch.zeros((n, h, w), dtype=torch.int16, device="cuda:0")
    planar = DeviceClip(mk(NSRC, c.h, c.w), mk(NSRC, c.h // 2, c.w // 2), mk(NSRC, c.h // 2, c.w // 2), c.w, c.h, c.bits)
    weave_fields(ctx, src.Y, src.U, None, planar, nv12=True, msb=True)
    out = DeviceClip(mk(len(PLAN), c.h, c.w), mk(len(PLAN), c.h // 2, c.w // 2), mk(len(PLAN), c.h // 2, c.w // 2), c.w, c.h, c.bits)
    kfm_render(ctx, planar, PLAN, out, deint="adaptive")
    torch.cuda.synchronize()
    got = download(dst_host, dst_flat)
    Y, UV = (dst_host.view(k, got)[:, :, :dst_host.geom[k][3]] for k in range(2))
    host = lambda t: t.cpu().numpy().view(np.uint16)
    assert np.array_equal(Y >> c.s, host(out.Y)) and np.array_equal(UV[:, :, 0::2] >> c.s, host(out.U)) and np.array_equal(UV[:, :, 1::2] >> c.s, host(out.V))
    low = (1 << c.s) - 1
    for k, e in enumerate(PLAN):
        for parity, frame in S.copied_rows(e, 0):
            assert np.array_equal(Y[k, parity::2], c.planes[0][frame, parity::2]) and np.array_equal(UV[k, parity::2], c.planes[1][frame, parity::2])
        ip = S.interpolated_rows(e)
        if ip is not None:
            assert not (Y[k, ip::2] & low).any() and not (UV[k, ip::2] & low).any()


def test_refusals_launch_nothing_and_python_takes_surfaces(gpu):
    from amatsukaze_amd import kfm_render
    ctx, torch = gpu
    W, H, N = 96, 36, NSRC
    clips = {}

    def pair(name, shape, nout=4):
        sh, dh = Surf(N, shape, rng=np.random.default_rng(len(name))), sentinel_surf(nout, shape)
        clips[name] = [(sh, *upload(gpu, sh)), (dh, *upload(gpu, dh))]
        return clips[name][0][1].ref(), clips[name][1][1].ref()

    nv12_s, nv12_d = pair("nv12", SHAPES["nv12-96x36-aligned"])
    pl8_s, pl8_d = pair("planar8", (W, H, 8, False, False, 96, 48, 0, 0, False))
    p010_s, p010_d = pair("p010", SHAPES["p010-96x36-aligned"])
    p012_s, p012_d = pair("p012", SHAPES["p012-96x36"])
    plan = lambda *e: R.plan_array(list(e))
    ok = plan((T_, 2, 2, 1))
    nv12_src = clips["nv12"][0][1]
    mid = GS.cut(nv12_src, 2, 5).ref()                                                       # frames 2..4 of a clip of 8
    cases = {
        # name: (arguments, a word the message must hold)
        "thresh 0": ((nv12_s, 0, N, N, W, H, ok, ADAPTIVE, 0, nv12_d), "thresh"),
        "thresh 3 on P010": ((p010_s, 0, N, N, W, H, ok, ADAPTIVE, 3, p010_d), "thresh"),
        "thresh -2": ((nv12_s, 0, N, N, W, H, ok, ADAPTIVE, -2, nv12_d), "thresh"),
        "deint 2": ((nv12_s, 0, N, N, W, H, ok, 2, -1, nv12_d), "deint"),
        "deint -1": ((p010_s, 0, N, N, W, H, ok, -1, -1, p010_d), "deint"),
        "BOB_TOP without frame n - 1": ((mid, 2, 3, 8, W, H, plan((W_, 3, 3, 2), (T_, 2, 2, 1)), ADAPTIVE, -1, nv12_d), "plan entry 1: the neighbour frame 1 "),
        "BOB_BOTTOM without frame n + 1": ((mid, 2, 3, 8, W, H, plan((B_, 4, 4, 1)), ADAPTIVE, -1, nv12_d), "plan entry 0: the neighbour frame 5 "),
        "NV12 into planes": ((nv12_s, 0, N, N, W, H, ok, ADAPTIVE, -1, pl8_d), "not in kind"),
        "planes into NV12": ((pl8_s, 0, N, N, W, H, ok, ADAPTIVE, -1, nv12_d), "not in kind"),
        "P010 into NV12": ((p010_s, 0, N, N, W, H, ok, ADAPTIVE, -1, nv12_d), "differ in bits"),
        "P010 into P012": ((p010_s, 0, N, N, W, H, ok, ADAPTIVE, -1, p012_d), "bits"),
        "P010 into a descriptor that says P012": ((p010_s, 0, N, N, W, H, ok, ADAPTIVE, -1, GS.changed(p010_d, bits=12)), "bits"),
        "destination is the source": ((nv12_s, 0, N, N, W, H, ok, ADAPTIVE, -1, nv12_s), "overlaps the source's"),
        "odd width": ((nv12_s, 0, N, N, W - 1, H, ok, ADAPTIVE, -1, nv12_d), "even"),
        "source pitchUV below width": ((GS.changed(nv12_s, pitchUV=W - 2), 0, N, N, W, H, ok, ADAPTIVE, -1, nv12_d), "source: pitch smaller than the row"),
        "negative destination stride": ((p010_s, 0, N, N, W, H, ok, ADAPTIVE, -1, GS.changed(p010_d, strideY=-p010_d.strideY)), "destination: negative frame stride"),
        "overlapping destination UV frames": ((nv12_s, 0, N, N, W, H, plan((T_, 2, 2, 1), (B_, 2, 2, 1)), ADAPTIVE, -1, GS.changed(nv12_d, strideUV=(H // 2) * nv12_d.pitchUV - 1)),
                                              "destination frames overlap each other"),
    }
    for what, (args, word) in cases.items():
        r, msg = raw_deint_surfaces(ctx, *args)
        assert r == 0 and msg.strip() and "KFMRender" in msg and word in msg, (what, msg)
    torch.cuda.synchronize()
    for name, both in clips.items():
        for host, _, flat_t in both:
            for g, a in zip(download(host, flat_t), host.flat):
                assert np.array_equal(g, a), name                                   # sources as they were, destinations still the sentinel
    # ... and from Python the same calls on DeviceSurfaces succeed: NV12 and P010
    for name, bits, msb in (("nv12", 8, False), ("p010", 10, True)):
        (sh, src, _), (dh, dst, dst_flat) = clips[name]
        kfm_render(ctx, src, PLAN[:4], dst, deint="adaptive")
        torch.cuda.synchronize()
        want, _ = AS.render_adaptive_surfaces_ref(sh.planes, PLAN[:4], bits, True, msb)
        assert_buffers(download(dh, dst_flat), expected_buffers(dh, want), name, "from Python")
