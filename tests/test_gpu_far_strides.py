"""Every kernel on batches whose frames lie more than 4 GiB apart: three 352 x 240 frames in the windows of tests/far_stride_clips.py, in
ONE allocation of about 12 GiB that the whole module shares (torch.empty writes nothing), handed to the C ABI as strided views.

Expected values always come from the CPU (far_stride_clips.Refs: the oracle and the numpy references) over the three true frames;
comparisons are byte for byte, the linear analysis modes by their own criterion (test_analyze_linear_mode_shapes).  A kernel that forms a
frame offset in 32 bits, in bytes or in samples, reads or writes a decoy window instead: wrong bytes, never a fault
(tests/test_far_stride_layout_host.py).  Writers also leave every decoy window of their destination and a 4 KiB band around every true
destination frame as they found them."""
import ctypes as C
import time

import numpy as np
import pytest

import far_stride_clips as F
import surface_clips as SC

pytestmark = pytest.mark.gpu

W, H, LW, LH, IMGX, IMGY = F.W, F.H, F.LW, F.LH, F.IMGX, F.IMGY
LAYOUTS = list(F.LAYOUTS)
OTHER = {"L31": "L32", "L32": "L31"}
PAIR, GENERIC = "logo_eval_pair_kernel.scan", "logo_eval_fused_kernel.scan"
RECORD = {"kernels": {}}                      # what ctx.profile reported per operation; printed when the module is done


class Far:
    """the allocation, and the windows of far_stride_clips in it"""

    def __init__(self, torch, dev):
        self.torch, self.dev, self.buf, self.alloc_error = torch, dev, None, None
        try:
            self.buf = torch.empty(F.A, dtype=torch.uint8, device=dev)
            self.buf16 = self.buf.view(torch.int16)
        except Exception as e:      # noqa: BLE001
            self.alloc_error = f"cannot allocate the {F.A} bytes ({F.A / F.GiB:.2f} GiB) of the far-stride tests in one piece: {e!r}"

    def _flat(self, es=1):
        assert self.buf is not None, self.alloc_error          # (a failure of the test that asks, not a skip)
        return self.buf if es == 1 else self.buf16

    def put(self, addr, a):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert 0 <= addr and addr + b.size <= F.A
        self._flat()[addr:addr + b.size].copy_(self.torch.from_numpy(b.copy()))

    def get(self, addr, nbytes):
        assert 0 <= addr and addr + nbytes <= F.A
        return self._flat()[addr:addr + nbytes].cpu().numpy()

    def place(self, slot, frames, decoys, off=0):
        """frames [N, rows, row] into the true windows of every layout the slot has, decoys[w] [1, rows, row] into its decoy window w"""
        for lay in F.slot_layouts(slot):
            for n, a in enumerate(F.true_windows(slot, lay)):
                self.put(a + off, frames[n])
        for w, a in F.decoy_windows(slot):
            self.put(a + off, decoys[w][0])

    def fill(self, kind):
        """the pictures of a kind (and its previous picture) into their slots"""
        p = F.pictures()[kind]
        if kind in ("p8", "p10"):
            for k in "YUV":
                self.place(kind + k, p["true"][k], [d[k] for d in p["decoy"]])
            self.put(F.slot_base("prev8" if kind == "p8" else "prev10"), p["prev"]["Y"][0])
        else:
            uv = p["true"]["Y"][0].nbytes
            self.place(kind, p["true"]["Y"], [d["Y"] for d in p["decoy"]])
            self.place(kind, p["true"]["U"], [d["U"] for d in p["decoy"]], off=uv)
            if kind == "p010":
                self.put(F.slot_base("prevP010"), F.surface_bytes(p["prev"], 0))

    def fill_destination(self, slots, frames, dtype):
        """frames (or zeros) into the true windows of destination slots, and a decoy pattern into their decoy windows"""
        for slot, fr in zip(slots, frames):
            pat = [np.full((1,) + fr.shape[1:], 0x5A + w, dtype) for w in range(len(F.DECOYS))]
            self.place(slot, fr, pat)

    def view(self, slot, layout, rows, pitch, es, off=0, n=F.N):
        """the (n, rows, pitch) tensor view of a slot's frames in a layout; off: bytes into the window"""
        addr = F.slot_base(slot) + off
        assert addr % es == 0 and F.STRIDES[layout] % es == 0 and layout in F.slot_layouts(slot)
        return self.torch.as_strided(self._flat(es), (n, rows, pitch), (F.STRIDES[layout] // es, pitch, 1), addr // es)

    def frames(self, slot, layout, rows, pitch, dtype, off=0):
        """the frames as they lie now: numpy [N, rows, pitch]"""
        nb = rows * pitch * np.dtype(dtype).itemsize
        return np.stack([self.get(a + off, nb).view(dtype).reshape(rows, pitch) for a in F.true_windows(slot, layout)])

    def watch(self, layout, extents):
        """{slot: bytes of its windows} -> the bytes a writer in `layout` must leave alone: the decoy windows, the other layout's frames,
        and GUARD bytes on both sides of every true frame"""
        regs = []
        for slot, ext in extents.items():
            regs += [(a, ext) for _, a in F.decoy_windows(slot)]
            regs += [(a, ext) for lay in F.slot_layouts(slot) if lay != layout for a in F.true_windows(slot, lay)[1:]]
            for a in F.true_windows(slot, layout):
                regs += [(a - F.GUARD, F.GUARD), (a + ext, F.GUARD)]
        return [(a, n, self.get(a, n)) for a, n in regs]

    def assert_unchanged(self, watched):
        for a, n, before in watched:
            assert np.array_equal(self.get(a, n), before), f"bytes [{a}, {a + n}) of the allocation were written"


@pytest.fixture(scope="module")
def env():
    import torch
    from amatsukaze_amd import Context, Logo
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dev = torch.device("cuda:0")
    t0 = time.time()
    ctx = Context(0)
    refs = F.Refs()
    far = Far(torch, dev)
    if far.buf is not None:
        for kind in F.KINDS:
            far.fill(kind)
        torch.cuda.synchronize()
    e = dict(torch=torch, dev=dev, ctx=ctx, lib=ctx.lib, far=far, refs=refs,
             logo=Logo.from_planes(ctx, refs.data, LW, LH, W, H, IMGX, IMGY), logo_big=Logo.from_planes(ctx, refs.big, LW, LH, W, H, IMGX, IMGY),
             d_fades=torch.from_numpy(F.FADES.copy()).to(dev))
    RECORD["setup_seconds"] = round(time.time() - t0, 3)
    yield e
    ctx.synchronize()
    print("far strides record:", {"allocation_bytes": F.A, **RECORD})
    far.buf16 = far.buf = None
    e.clear()
    torch.cuda.empty_cache()


def profiled(env, name, run):
    """runs run() under the context's profile and records the kernels it launched"""
    ctx = env["ctx"]
    ctx.profile(True)
    try:
        out = run()
        ctx.synchronize()
        used = sorted(k for k, (calls, _) in ctx.profile_report().items() if calls)
    finally:
        ctx.profile(False)
    RECORD["kernels"].setdefault(name, used)
    return out, used


def es_of(bits):
    return 1 if bits <= 8 else 2


def dt_of(bits):
    return np.uint8 if bits <= 8 else np.uint16


def planar_clip(env, kind, layout, slots=None):
    from amatsukaze_amd import DeviceClip
    bits = F.BITS[kind]
    es = es_of(bits)
    sl = slots or [kind + k for k in "YUV"]
    far = env["far"]
    return DeviceClip(far.view(sl[0], layout, H, W, es), far.view(sl[1], layout, H // 2, W // 2, es), far.view(sl[2], layout, H // 2, W // 2, es),
                      width=W, height=H, bits=bits)


def surfaces(env, kind, layout, slot=None, n=F.N):
    from amatsukaze_amd.api import DeviceSurfaces
    bits = F.BITS[kind]
    es = es_of(bits)
    far, slot = env["far"], slot or kind
    return DeviceSurfaces(far.view(slot, layout, H, W, es, n=n), far.view(slot, layout, H // 2, W, es, off=H * W * es, n=n), None, W, H, bits,
                          interleaved=True, msb=(kind == "p010"))


def planar_frames(env, kind, layout, slots=None):
    dt = dt_of(F.BITS[kind])
    sl = slots or [kind + k for k in "YUV"]
    far = env["far"]
    return [far.frames(sl[0], layout, H, W, dt), far.frames(sl[1], layout, H // 2, W // 2, dt), far.frames(sl[2], layout, H // 2, W // 2, dt)]


def surface_frames(env, kind, layout, slot=None):
    dt = dt_of(F.BITS[kind])
    far, slot = env["far"], slot or kind
    return [far.frames(slot, layout, H, W, dt), far.frames(slot, layout, H // 2, W, dt, off=H * W * np.dtype(dt).itemsize)]


def planar_extents(kind, slots):
    es = es_of(F.BITS[kind])
    return {slots[0]: H * W * es, slots[1]: (H // 2) * (W // 2) * es, slots[2]: (H // 2) * (W // 2) * es}


def assert_planes(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        w = np.asarray(w)
        assert g.shape == w.shape and np.array_equal(g, w.astype(g.dtype)), (what, "plane", k, "first frame that differs",
                                                                             int(np.argmax([(g[n] != w[n]).any() for n in range(len(g))])))


# ---------------------------------------------------------------------------------------------------------------- analysis
def linear_criterion(env, an, got, want, bits):
    """test_analyze_linear_mode_shapes: scores within 1e-4 and inside the library's bound, fades identical"""
    from amatsukaze_amd import AMTEraseLogo
    err = np.abs(got - want)
    tol = 1e-4 * np.maximum(1.0, np.abs(want))
    assert (err <= tol).all(), float(err.max())
    for k in range(3):
        assert err[:, 11 * k:11 * k + 11].max() <= an.error_bound(k, bits) * max(1.0, float(np.abs(want).max()))
    er = AMTEraseLogo(env["ctx"], env["logo"], "", 0, 16)
    assert er.calc_fades(got, F.N).tobytes() == er.calc_fades(want, F.N).tobytes()


def run_analysis(env, mode, bits, layout):
    from amatsukaze_amd import AMTAnalyzeLogo
    torch = env["torch"]
    an = AMTAnalyzeLogo(env["ctx"], env["logo"], 0.35, mode=mode, sentinels=1 if mode == "monitored" else 16)
    Y = env["far"].view(f"p{bits}Y", layout, H, W, es_of(bits))
    out = torch.zeros((F.N, 33), dtype=torch.float32, device=env["dev"])
    profiled(env, f"analyze-{mode}-{bits}", lambda: an.analyze_device(Y, bits, out))
    return an, out.cpu().numpy()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("mode", ["exact", "linear_unguarded", "linear", "monitored"])
def test_analyze(env, mode, bits, layout):
    want = env["refs"].analyze(F.pictures()[f"p{bits}"]["true"], bits)
    an, got = run_analysis(env, mode, bits, layout)
    if mode == "exact":
        assert got.tobytes() == want.tobytes()
        return
    linear_criterion(env, an, got, want, bits)
    if mode == "monitored":                                   # (one sentinel per batch: frame 0 carries the exact record)
        assert got[0].tobytes() == want[0].tobytes() and not an.monitor_stats()["downgraded"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", ["linear", "monitored"])
def test_analyze_hands_the_far_frame_with_a_sample_above_maxv_to_the_exact_kernel(env, mode, layout):
    """frame 2 holds one sample above maxv inside the rectangle: rect_range_flag lists it and the listed exact re-evaluation (scatter,
    frame count on the device) writes its record -- the exact mode's bytes"""
    far = env["far"]
    p10 = F.pictures()["p10"]
    hot = F.with_hot_sample(p10["true"])
    want = env["refs"].analyze(hot, 10)
    try:
        for lay in F.LAYOUTS:
            far.put(F.true_windows("p10Y", lay)[2], hot["Y"][2])
        an, got = run_analysis(env, mode, 10, layout)
        assert got[2].tobytes() == want[2].tobytes()
        assert an.last_refined() >= 1
        linear_criterion(env, an, got, want, 10)
    finally:
        far.fill("p10")


# ---------------------------------------------------------------------------------------------------------------- scan
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("generic", [False, True], ids=["pair", "generic"])
def test_logoframe_scan_batch(env, generic, bits, layout):
    from amatsukaze_amd import LogoFrame
    lf = LogoFrame(env["ctx"], [env["logo_big"] if generic else env["logo"]], 0.35)
    lf.begin(W, H, bits, F.N)
    Y = env["far"].view(f"p{bits}Y", layout, H, W, es_of(bits))
    _, used = profiled(env, f"scan-{'generic' if generic else 'pair'}-{bits}", lambda: lf.scan_batch(Y, bits, 0))
    assert used == [GENERIC if generic else PAIR], used
    want = env["refs"].scan(F.pictures()[f"p{bits}"]["true"], bits, generic)
    assert np.isfinite(want).all()
    assert lf.evalResults.tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------------------------- Delogo
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["p8", "p10"])
@pytest.mark.parametrize("form", ["in_place", "to_destination", "rectangle_only"])
def test_erase_planar(env, form, kind, layout):
    from amatsukaze_amd import AMTEraseLogo
    far, bits = env["far"], F.BITS[kind]
    es, dt = es_of(bits), dt_of(bits)
    true = F.pictures()[kind]["true"]
    want = list(env["refs"].erase(true, bits).values())
    er = AMTEraseLogo(env["ctx"], env["logo"])
    src_slots, dst_slots = [kind + k for k in "YUV"], ["dstY", "dstU", "dstV"]
    try:
        if form == "to_destination":                     # (one stride serves both batches in the ABI: the destination is in the same layout)
            far.fill_destination(dst_slots, [true[k] for k in "YUV"], dt)
            watched = far.watch(layout, planar_extents(kind, dst_slots))
            profiled(env, f"erase-{form}-{bits}", lambda: er.erase_device_fades(planar_clip(env, kind, layout), env["d_fades"],
                                                                                dst=planar_clip(env, kind, layout, dst_slots)))
            assert_planes(planar_frames(env, kind, layout, dst_slots), want, form)
            assert_planes(planar_frames(env, kind, layout), [true[k] for k in "YUV"], "the source")
        else:
            watched = far.watch(layout, planar_extents(kind, src_slots))
            if form == "in_place":
                profiled(env, f"erase-{form}-{bits}", lambda: er.erase_device_fades(planar_clip(env, kind, layout), env["d_fades"]))
            else:                                        # planes that hold only the rectangle: here the rectangle of the far frames
                cx, cy = IMGX // 2, IMGY // 2
                Y = far.view(src_slots[0], layout, LH, W, es, off=(IMGY * W + IMGX) * es)
                U = far.view(src_slots[1], layout, LH // 2, W // 2, es, off=(cy * (W // 2) + cx) * es)
                V = far.view(src_slots[2], layout, LH // 2, W // 2, es, off=(cy * (W // 2) + cx) * es)
                profiled(env, f"erase-{form}-{bits}", lambda: er.erase_rect(Y, U, V, bits, F.FADES))
            assert_planes(planar_frames(env, kind, layout), want, form)
        far.assert_unchanged(watched)
    finally:
        far.fill(kind)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["nv12", "p010"])
def test_erase_surfaces_in_place(env, kind, layout):
    from amatsukaze_amd import AMTEraseLogo
    far, bits = env["far"], F.BITS[kind]
    true = F.pictures()[kind]["true"]
    want = env["refs"].erase_surfaces(true, bits, kind == "p010")
    er = AMTEraseLogo(env["ctx"], env["logo"])
    assert er.rect == (IMGX, IMGY, LW, LH, 1)
    try:
        watched = far.watch(layout, {kind: F.window_extent(kind)})
        profiled(env, f"erase_surfaces-{kind}", lambda: er.erase_surfaces(surfaces(env, kind, layout), d_fades=env["d_fades"]))
        assert_planes(surface_frames(env, kind, layout), [want["Y"], want["U"]], kind)
        far.assert_unchanged(watched)
    finally:
        far.fill(kind)


# ---------------------------------------------------------------------------------------------------------------- LogoScan
@pytest.mark.parametrize("layout", LAYOUTS)
def test_logoscan_add_batch_and_sums(env, layout):
    """scan_border and scan_accumulate: AddFrame's verdicts and the exact integer sums"""
    from amatsukaze_amd import LogoScan
    scan = LogoScan(env["ctx"], LW, LH, F.THY)
    (valid, nacc), _ = profiled(env, "logoscan", lambda: scan.add_batch(planar_clip(env, "p8", layout), IMGX, IMGY))
    want_valid, osum = env["refs"].logoscan(F.pictures()["p8"]["true"])
    assert valid.tolist() == want_valid.tolist() == [1] * F.N and nacc == F.N == scan.nframes
    s, p = scan.sums()
    s = s.reshape(-1, 3)
    for col, ocol in ((0, 0), (1, 2), (2, 4)):                                   # sumF, sumF2, sumFB
        assert np.array_equal(s[:, col], osum[:, ocol].astype(np.int64)), col
    assert p[0] == int(osum[0, 1]) and p[1] == int(osum[0, 3])
    assert p[2] == int(osum[LW * LH, 1]) and p[4] == int(osum[LW * LH + (LW // 2) * (LH // 2), 1])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("feed", ["planar", "surfaces"])
def test_scanlogo_stream_session(env, tmp_path, feed, layout):
    """the same far batch fed twice fills a quota of six (scan_keep copies the kept rectangles out of the far frames); the .lgd is the
    oracle's ScanLogo over the three frames twice"""
    from amatsukaze_amd import ScanLogoStream
    ctx = env["ctx"]
    rounds = 2
    want = env["refs"].scanlogo_lgd(F.pictures()["p8"]["true"], rounds, tmp_path / "orc.lgd")
    st = ScanLogoStream(ctx, W, H, IMGX, IMGY, LW, LH, F.THY, F.N * rounds)

    def run():
        for r in range(rounds):
            if feed == "planar":
                nkept, done = st.feed(planar_clip(env, "p8", layout))
            else:
                nkept, done = st.feed_surfaces(surfaces(env, "nv12", layout))
            assert nkept == F.N * (r + 1) and done == (r == rounds - 1)

    profiled(env, f"scanlogo_stream-{feed}", run)
    dst = tmp_path / "gpu.lgd"
    assert st.finish(1041, dst), ctx.lib.amtgpu_last_error(ctx.h)
    assert dst.read_bytes() == want


@pytest.mark.parametrize("layout", LAYOUTS)
def test_surfaces_extract_rect_to_far_planes(env, layout):
    """the rectangle of far P010 surfaces as planar LSB planes that lie far apart as well (the other layout)"""
    far, ctx = env["far"], env["ctx"]
    dl = OTHER[layout]
    dslots = ["dstY", "dstU", "dstV"]
    want = list(SC.crop(SC.from_surfaces(F.pictures()["p010"]["true"], W, H, 10, True, True), IMGX, IMGY, LW, LH).values())
    far.fill_destination(dslots, [np.zeros_like(w) for w in want], np.uint16)
    ext = {"dstY": LW * LH * 2, "dstU": (LW // 2) * (LH // 2) * 2, "dstV": (LW // 2) * (LH // 2) * 2}
    watched = far.watch(dl, ext)
    Y, U, V = far.view("dstY", dl, LH, LW, 2), far.view("dstU", dl, LH // 2, LW // 2, 2), far.view("dstV", dl, LH // 2, LW // 2, 2)
    d = surfaces(env, "p010", layout).ref()
    profiled(env, "extract_rect-p010", lambda: ctx.check(ctx.lib.amtgpu_surfaces_extract_rect(
        ctx.h, C.byref(d), IMGX, IMGY, LW, LH, F.N, C.c_void_p(Y.data_ptr()), C.c_void_p(U.data_ptr()), C.c_void_p(V.data_ptr()),
        int(Y.stride(0)) * 2, int(U.stride(0)) * 2, int(Y.stride(1)), int(U.stride(1))), "extract_rect"))
    got = [far.frames("dstY", dl, LH, LW, np.uint16), far.frames("dstU", dl, LH // 2, LW // 2, np.uint16),
           far.frames("dstV", dl, LH // 2, LW // 2, np.uint16)]
    assert_planes(got, want, "extract_rect")
    far.assert_unchanged(watched)


# ---------------------------------------------------------------------------------------------------------------- whole-frame passes
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["p8", "p10", "p010"])
def test_frame_stats(env, kind, layout):
    from amatsukaze_amd import FrameStats
    torch, far, bits = env["torch"], env["far"], F.BITS[kind]
    p = F.pictures()[kind]
    shift = 6 if kind == "p010" else 0
    want = env["refs"].frame_stats(p["true"]["Y"], p["prev"]["Y"], shift)
    fs = FrameStats(env["ctx"], W, H, bits)
    out = torch.zeros((F.N, 8), dtype=torch.int64, device=env["dev"])
    if kind == "p010":
        prev = surfaces(env, "p010", layout, slot="prevP010", n=1)
        profiled(env, f"frame_stats-{kind}", lambda: fs.run_device_surfaces(surfaces(env, kind, layout), out, prev))
    else:
        es = es_of(bits)
        prevY = far.view("prev8" if kind == "p8" else "prev10", layout, H, W, es, n=1)
        profiled(env, f"frame_stats-{kind}", lambda: fs.run_device(far.view(kind + "Y", layout, H, W, es), out, prevY=prevY))
    assert np.array_equal(out.cpu().numpy().astype(np.uint64), want)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["p8", "p10", "p010"])
def test_logo_finder(env, kind, layout):
    """amtgpu_logofind_add_batch at 8 and 16 bits, amtgpu_logofind_add_surfaces on P010"""
    from amatsukaze_amd.api import LogoFinder
    far = env["far"]
    want = env["refs"].logofind(F.pictures()[kind]["true"]["Y"], 6 if kind == "p010" else 0)
    finder = LogoFinder(env["ctx"], W, H, {"p8": 8, "p10": 16, "p010": 10}[kind])
    if kind == "p010":
        profiled(env, f"logofind-{kind}", lambda: finder.add_surfaces(surfaces(env, kind, layout)))
    else:
        profiled(env, f"logofind-{kind}", lambda: finder.add_device(far.view(kind + "Y", layout, H, W, es_of(F.BITS[kind]))))
    S1, SM = finder.sums()
    assert finder.nframes == F.N
    assert np.array_equal(np.concatenate([S1.ravel(), SM.ravel()]), want)


# ---------------------------------------------------------------------------------------------------------------- weave and render
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["p8", "p10", "nv12", "p010"])
def test_weave_fields(env, kind, layout):
    """planar, nv12=True and msb=True (P010): far pictures in one layout, far frames out in the other"""
    from amatsukaze_amd import DeviceClip
    from amatsukaze_amd.api import weave_fields
    far, bits = env["far"], F.BITS[kind]
    es, dt, dl = es_of(bits), dt_of(bits), OTHER[layout]
    nv12, msb = kind in ("nv12", "p010"), kind == "p010"
    true = F.pictures()[kind]["true"]
    want = env["refs"].weave(true, nv12, 6 if msb else 0)
    dslots = ["dstY", "dstU", "dstV"]
    far.fill_destination(dslots, [np.zeros_like(w) for w in want], dt)
    okind = "p8" if bits == 8 else "p10"
    watched = far.watch(dl, planar_extents(okind, dslots))
    dst = planar_clip(env, okind, dl, dslots)
    if nv12:
        s = surfaces(env, kind, layout)
        srcY, srcU, srcV = s.Y, s.U, None
    else:
        c = planar_clip(env, kind, layout)
        srcY, srcU, srcV = c.Y, c.U, c.V
    profiled(env, f"weave-{kind}", lambda: weave_fields(env["ctx"], srcY, srcU, srcV, dst, F.WEAVE_TOP, F.WEAVE_BOTTOM, nv12=nv12, msb=msb))
    assert_planes(planar_frames(env, okind, dl, dslots), want, kind)
    far.assert_unchanged(watched)


# The renderer refuses batches whose byte ranges touch, so two far batches of one allocation have to lie one behind the other: L31 frames
# render to a second L31 batch behind them; an L32 batch has no room for a second one under the cap and is rendered to, and from, near frames.
RENDER_ROUTES = {"L31_to_L31": ("L31", None, "L31", "rd"), "L32_to_near": ("L32", None, "near", "near"), "near_to_L32": ("near", "near", "L32", "dst")}


@pytest.mark.parametrize("route", RENDER_ROUTES)
@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("deint,thresh", F.RENDER_MODES, ids=[f"{d}{t}" for d, t in F.RENDER_MODES])
def test_kfm_render(env, deint, thresh, kind, route):
    """a woven frame across frames 2 and 1 and both bobs of frame 1, in kind: every source frame is read, frames 0 and 2 as neighbours"""
    from amatsukaze_amd.api import kfm_render
    far, bits = env["far"], F.BITS[kind]
    dt = dt_of(bits)
    sl, sprefix, dl, dprefix = RENDER_ROUTES[route]
    true = F.pictures()[kind]["true"]
    want = list(env["refs"].render(kind, true, deint, thresh))
    if kind in ("p8", "p10"):
        dslots = [dprefix + k for k in "YUV"]
        sslots = [sprefix + k for k in "YUV"] if sprefix else None
        if sslots:
            far.fill_destination(sslots, [true[k] for k in "YUV"], dt)
        far.fill_destination(dslots, [np.zeros_like(w) for w in want], dt)
        watched = far.watch(dl, planar_extents(kind, dslots))
        src, dst = planar_clip(env, kind, sl, sslots), planar_clip(env, kind, dl, dslots)
        read = lambda: planar_frames(env, kind, dl, dslots)
    else:
        if sprefix:
            far.fill_destination([sprefix + "S"], [np.concatenate([true["Y"], true["U"]], axis=1)], dt)
        zero = np.zeros((F.N, H + H // 2, W), dt)
        far.fill_destination([dprefix + "S"], [zero], dt)
        watched = far.watch(dl, {dprefix + "S": zero[0].nbytes})
        src, dst = surfaces(env, kind, sl, slot=sprefix + "S" if sprefix else None), surfaces(env, kind, dl, slot=dprefix + "S")
        read = lambda: surface_frames(env, kind, dl, slot=dprefix + "S")
    profiled(env, f"render-{deint}{thresh}-{kind}", lambda: kfm_render(env["ctx"], src, F.PLAN, dst, thresh=thresh, deint=deint))
    assert_planes(read(), want, (kind, deint, thresh, route))
    far.assert_unchanged(watched)


# ---------------------------------------------------------------------------------------------------------------- row copies
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("registered", [False, True], ids=["ring", "registered"])
def test_frames_upload_strided(env, registered, layout):
    """three chunks -- whole 8-bit luma frames -- to places a far frame stride apart; from a registered host range ingest_rows_kernel
    reads the host memory itself"""
    torch, far, ctx, lib = env["torch"], env["far"], env["ctx"], env["lib"]
    Y = F.pictures()["p8"]["true"]["Y"]
    chunk = Y[0].nbytes
    host = np.zeros((F.N, chunk + 256), np.uint8)                     # (a host stride that is not the chunk)
    host[:, :chunk] = Y.reshape(F.N, -1)
    far.fill_destination(["dstY"], [np.zeros_like(Y)], np.uint8)
    watched = far.watch(layout, {"dstY": chunk})
    torch.cuda.synchronize()                                          # (uploads run on the context's side stream)
    if registered:
        ctx.check(lib.amtgpu_frames_register(ctx.h, C.c_void_p(host.ctypes.data), host.size))
    try:
        ctx.check(lib.amtgpu_frames_upload_strided(ctx.h, C.c_void_p(far.buf.data_ptr() + F.slot_base("dstY")), F.LAYOUTS[layout],
                                                   C.c_void_p(host.ctypes.data), host.strides[0], chunk, F.N))
        ctx.check(lib.amtgpu_frames_upload_wait(ctx.h))
        ctx.synchronize()
        torch.cuda.synchronize()
    finally:
        if registered:
            ctx.check(lib.amtgpu_frames_unregister(ctx.h, C.c_void_p(host.ctypes.data)))
    assert_planes([far.frames("dstY", layout, H, W, np.uint8)], [Y], "upload_strided")
    far.assert_unchanged(watched)


# ---------------------------------------------------------------------------------------------------------------- audio
def test_audio_levels_past_element_2_31(env):
    """the allocation as ONE int16 tensor: the PCM of three video frames starts at element 2^31 + 10 Mi of it (byte 2^32 + 20 Mi); decoy PCM
    lies where the sign-extended element offset and the truncated byte offset point"""
    from amatsukaze_amd.api import AudioLevels
    far, ctx = env["far"], env["ctx"]
    true = F.pcm(1)
    far.put(F.PCM_TRUE, true)
    for k, (name, addr) in enumerate(sorted(F.PCM_DECOYS.items())):
        far.put(addr, F.pcm(2 + k))
    first = F.PCM_BASE // 2
    tensor = far._flat(2)[first:first + F.PCM_NUMEL]
    assert tensor.is_contiguous() and tensor.numel() > 1 << 31
    al = AudioLevels(ctx, F.SAMPLE_RATE, F.CHANNELS, *F.FPS, F.PCM_START + F.PCM_FRAMES)
    out, _ = profiled(env, "audio_levels", lambda: al.run_device(tensor, F.PCM_FIRST, F.AUDIO_FIRST_FRAME, F.N))
    assert np.array_equal(out.cpu().numpy().astype(np.uint64), F.audio_ref(true))
