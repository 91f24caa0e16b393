"""The encode-time chain on decoder surfaces where they lie (NV12, P010 / P012, planar MSB): delogo_surfaces_kernel on every access
width and layout against the CPU oracle over whole planes -- pitch padding, untouched frames and the low bits of untouched MSB containers
included (tests/surface_erase_ref.py, pinned by test_surface_erase_ref_host.py) -- then AMTAnalyzeLogo.analyze_surfaces ->
calc_fades_device -> erase_surfaces and LogoFrame.scan_surfaces against the same calls on the planar clip, byte for byte, and what the
entry points must refuse."""
import ctypes as C

import numpy as np
import pytest

import amt_synth as S
import surface_clips as SC
import surface_erase_ref as ER
from amtlib import Oracle
from test_gpu_erase_shapes import LOGOS, assert_finite_mix, fades_for, host, make_planes, to_dev
from test_gpu_parity import SMALL, gpu, make_case  # noqa: F401  (gpu: fixture)

pytestmark = pytest.mark.gpu

LAYOUTS = [(8, 1, 0), (10, 1, 1), (12, 1, 1), (16, 1, 1), (10, 0, 1), (10, 1, 0), (10, 0, 0)]        # (bits, interleaved, msb)
LAYOUT_IDS = ["%d-%s-%s" % (b, "il" if i else "planar", "msb" if m else "lsb") for b, i, m in LAYOUTS]
# W, H, LW, LH, IMGX, IMGY, luma pitch - W, chroma pitch - W/2 (interleaved: UV pitch - W), plane base offset in containers
ODD_PAIR = (352, 240, 66, 40, 226, 18, 32, 16, 0)           # cx = 113: the interleaved row starts on an odd pair (container 226)
BODIES = {k: LOGOS[k] for k in ("100x34_y16", "98x50_y18", "98x50_y16", "520x18", "96x48_odd_luma_pitch", "96x48_base_plus_1")}
BODIES["66x40_odd_pair"] = ODD_PAIR


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def fill_of(bits):
    return 0xA5 if bits == 8 else 0xA5A5


def device_surfaces(gpu, surf, W, H, bits, interleaved, msb, off=0):
    from amatsukaze_amd import DeviceSurfaces
    return DeviceSurfaces(to_dev(gpu, surf["Y"], off), to_dev(gpu, surf["U"], off), to_dev(gpu, surf["V"], off) if surf["V"] is not None else None,
                          width=W, height=H, bits=bits, interleaved=bool(interleaved), msb=bool(msb))


def assert_surfaces(d, want, what):
    for k in "YUV":
        t = getattr(d, k)
        if t is None:
            assert want[k] is None
            continue
        got = host(t)
        if not np.array_equal(got, want[k]):
            f, y, x = (int(v[0]) for v in np.nonzero(got != want[k]))
            raise AssertionError(f"{what}: plane {k} frame {f} row {y} container {x}: kernel {got[f, y, x]:#x}, expected {want[k][f, y, x]:#x}, "
                                 f"{int((got != want[k]).sum())} containers differ")


def build(gpu, orc, geom, layout, n, data=None, seed=0):
    from amatsukaze_amd import AMTEraseLogo, Logo
    bits, il, msb = layout
    W, H, LW, LH, X, Y0, padY, padUV, off = geom
    maxv = (1 << bits) - 1
    if data is None:
        data = S.make_logo(LW, LH)[0]
    rs = np.random.RandomState(1000 * bits + n + seed + 7 * il + 3 * msb)
    planes = make_planes(rs, n, W, H, W, W // 2, bits, (X, Y0, LW, LH))
    if msb:
        planes = {k: np.minimum(v, maxv).astype(v.dtype) for k, v in planes.items()}      # an MSB sample cannot exceed maxv
    else:
        assert bits in (8, 16) or max(int(v.max()) for v in planes.values()) > maxv         # LSB containers keep values above it
    fades = fades_for(n)
    assert_finite_mix(data, LW, LH, planes, (X, Y0), fades, maxv)
    surf = SC.to_surfaces(planes, bits, il, msb, np.random.default_rng(seed + bits), padY, padUV, fill_of(bits))
    er = AMTEraseLogo(gpu["ctx"], Logo.from_planes(gpu["ctx"], data, LW, LH, W, H, X, Y0))
    lo = orc.make_logo(data, LW, LH, W, H, X, Y0)
    want = ER.expected_surfaces(orc, lo, surf, W, H, bits, il, msb, (X, Y0, LW, LH), fades, er.rect[4])
    live = ER.rewritten_frames(fades, bits, msb, er.rect[4])
    assert live.any() and not np.array_equal(want["Y"], surf["Y"]) and not np.array_equal(want["U"], surf["U"])
    return dict(W=W, H=H, layout=layout, off=off, surf=surf, want=want, fades=fades, er=er, live=live)


def run_both_entries(gpu, cs):
    """erase_surfaces(src, d_fades, dst): dst == expected over whole planes and src untouched; then erase_surfaces(src, fades) in place"""
    torch = gpu["torch"]
    src = device_surfaces(gpu, cs["surf"], cs["W"], cs["H"], *cs["layout"], off=cs["off"])
    dst = device_surfaces(gpu, cs["surf"], cs["W"], cs["H"], *cs["layout"], off=cs["off"])
    d_fades = torch.from_numpy(cs["fades"]).to(gpu["dev"])
    cs["er"].erase_surfaces(src, d_fades=d_fades, dst=dst)
    gpu["ctx"].synchronize()
    assert_surfaces(dst, cs["want"], "erase_surfaces(d_fades, dst)")
    assert_surfaces(src, cs["surf"], "erase_surfaces(d_fades, dst) source")
    cs["er"].erase_surfaces(src, fades=cs["fades"])
    gpu["ctx"].synchronize()
    assert_surfaces(src, cs["want"], "erase_surfaces(fades) in place")


# ---- a. every body, 27 frames ----
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", sorted(BODIES))
def test_erase_surfaces_every_body_27_frames(gpu, orc, name, layout):
    cs = build(gpu, orc, BODIES[name], layout, 27)
    assert cs["er"].rect[4] == 1
    bits, il, msb = layout
    # group 0 is all {0, 0}: untouched where fade 0 is skipped, computed (LSB 10-bit containers above maxv are clamped) elsewhere
    assert (cs["fades"][:8] == 0).all() and cs["live"][:8].any() == (not ER.skips_fade0(bits, msb, 1))
    run_both_entries(gpu, cs)


# ---- b. short batches ----
@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", ["98x50_y18", "100x34_y16"])
def test_erase_surfaces_short_batches(gpu, orc, name, layout, n):
    run_both_entries(gpu, build(gpu, orc, BODIES[name], layout, n))


# ---- c. frame corners ----
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("corner", ["origin", "bottom_right"])
def test_erase_surfaces_at_the_frame_corners(gpu, orc, corner, layout):
    """an unpadded surface with the rectangle at (0, 0) and flush with the last container of every plane"""
    W, H = 352, 240
    x, y = (0, 0) if corner == "origin" else (W - 96, H - 48)
    run_both_entries(gpu, build(gpu, orc, (W, H, 96, 48, x, y, 0, 0, 0), layout, 1))


# ---- d. a logo whose fade 0 is not the identity ----
def test_erase_surfaces_logo_whose_fade0_is_not_the_identity(gpu, orc):
    """the coefficients of test_erase_logo_whose_fade0_is_not_the_identity on P010: {0, 0} frames are computed and rewritten, low bits zero"""
    bits, il, msb = layout = (10, 1, 1)
    geom = LOGOS["98x50_y18"]
    W, H, LW, LH, X, Y0 = geom[:6]
    maxv = (1 << bits) - 1
    data = S.make_logo(LW, LH)[0].copy()
    ysz, csz = LW * LH, (LW // 2) * (LH // 2)
    for a_off, sz, pw in ((0, ysz, LW), (2 * ysz, csz, LW // 2), (2 * ysz + 2 * csz, csz, LW // 2)):
        for (r, c) in ((3, 1), (3, 2), (10, pw - 1), (11, 0), (20, 17)):
            data[a_off + r * pw + c] = np.float32(1e30)
            data[a_off + sz + r * pw + c] = np.float32(-1e30) * np.float32(200) / np.float32(maxv)
    cs = build(gpu, orc, geom, layout, 27, data=data, seed=9)
    assert cs["er"].rect == (X, Y0, LW, LH, 0)
    assert (cs["fades"][:8] == 0).all() and cs["live"].all()
    low = (1 << (16 - bits)) - 1
    assert np.all(cs["want"]["Y"][0, Y0:Y0 + LH, X:X + LW] & low == 0) and np.all(cs["surf"]["Y"][0, Y0:Y0 + LH, X:X + LW] & low != 0)
    run_both_entries(gpu, cs)


# ---- e. the chain, f. the LogoFrame scan: P010 and NV12 surfaces of the parity suite's small clip ----
def chain_case(gpu, bits):
    cs = make_case(gpu, SMALL, bits=bits, pitch_pad=32)
    W, H = SMALL["W"], SMALL["H"]
    msb = 1 if bits > 8 else 0
    tight = {"Y": cs["clip"]["Y"][:, :, :W], "U": cs["clip"]["U"][:, :, :W // 2], "V": cs["clip"]["V"][:, :, :W // 2]}
    assert max(int(v.max()) for v in tight.values()) <= (1 << bits) - 1
    surf = SC.to_surfaces(tight, bits, 1, msb, np.random.default_rng(bits), 32, 32, fill_of(bits))
    if msb:
        assert np.all(surf["Y"][:, :, :W] & ((1 << (16 - bits)) - 1) != 0)
    return cs, tight, surf, device_surfaces(gpu, surf, W, H, bits, 1, msb)


@pytest.mark.parametrize("mode", ["exact", "linear"])
@pytest.mark.parametrize("bits", [10, 8])
def test_chain_on_surfaces_equals_the_planar_chain(gpu, bits, mode):
    from amatsukaze_amd import AMTAnalyzeLogo, AMTEraseLogo
    torch = gpu["torch"]
    cs, tight, surf, ds = chain_case(gpu, bits)
    W, H, n = SMALL["W"], SMALL["H"], SMALL["N"]
    an = AMTAnalyzeLogo(gpu["ctx"], cs["logo"], 0.35, mode=mode)
    er = AMTEraseLogo(gpu["ctx"], cs["logo"])
    # surfaces: analyse -> decide -> erase, stream-ordered, no synchronise in between
    rec_s = an.analyze_surfaces(ds)
    fades_s = er.calc_fades_device(rec_s, n)
    er.erase_surfaces(ds, d_fades=fades_s)
    # the planar chain on the same pictures
    rec_p = torch.empty((n, 33), dtype=torch.float32, device=gpu["dev"])
    an.analyze_device(cs["dclip"].Y, bits, rec_p)
    fades_p = er.calc_fades_device(rec_p, n)
    er.erase_device_fades(cs["dclip"], fades_p)
    gpu["ctx"].synchronize()
    assert rec_s.shape == (n, 33) and rec_s.cpu().numpy().tobytes() == rec_p.cpu().numpy().tobytes()
    f_s, f_p = fades_s.cpu().numpy(), fades_p.cpu().numpy()
    assert f_s.tobytes() == f_p.tobytes() and (f_s != 0).any()
    got = SC.from_surfaces({k: (None if getattr(ds, k) is None else host(getattr(ds, k))) for k in "YUV"}, W, H, bits, 1, 1 if bits > 8 else 0)
    for k in "YUV":
        planar = host(getattr(cs["dclip"], k))[:, :, :got[k].shape[2]]
        assert np.array_equal(got[k], planar), k
        assert not np.array_equal(got[k], tight[k]) or k != "Y"              # the erase changed the luma


@pytest.mark.parametrize("bits", [10, 8])
def test_logoframe_scan_surfaces_equals_scanframes(gpu, bits):
    from amatsukaze_amd import DeviceSurfaces, Logo, LogoFrame
    cs, tight, surf, ds = chain_case(gpu, bits)
    cfg, ctx = SMALL, gpu["ctx"]
    W, H, n = cfg["W"], cfg["H"], cfg["N"]
    d2 = S.make_logo(cfg["LW"], cfg["LH"], seed=0x10600002, strength=0.5)[0]
    logo2 = Logo.from_planes(ctx, d2, cfg["LW"], cfg["LH"], W, H, cfg["IMGX"] - 30, cfg["IMGY"] + 10)
    top = Logo.from_planes(ctx, cs["data"], cfg["LW"], cfg["LH"], W, H, cfg["IMGX"], 0)        # a band that starts at the plane's first row
    for logos in ([cs["logo"], logo2], [top]):
        want = LogoFrame(ctx, logos, 0.35)
        want.scanFrames(cs["dclip"], batch=17)
        lf = LogoFrame(ctx, logos, 0.35)
        lf.begin(W, H, bits, n)
        for f0 in range(0, n, 17):                                            # ragged batches: 17, 17, 6
            lf.scan_surfaces(DeviceSurfaces(ds.Y[f0:f0 + 17], ds.U[f0:f0 + 17], None, W, H, bits, True, ds.msb), f0)
        got, ref = lf.evalResults, want.evalResults
        assert got.shape == (n, len(logos), 2) and got.tobytes() == ref.tobytes()
        assert np.isfinite(got).all() and len(np.unique(got[:, 0, 0])) > 1


# ---- g. refusals ----
def refused(gpu, ok, text):
    assert ok == 0
    msg = gpu["ctx"].lib.amtgpu_last_error(gpu["ctx"].h).decode()
    assert text in msg, msg


def test_surface_entry_points_refuse(gpu):
    from amatsukaze_amd import AMTAnalyzeLogo, AMTEraseLogo, DeviceSurfaces, LogoFrame, binding
    torch, ctx = gpu["torch"], gpu["ctx"]
    lib = ctx.lib
    cfg = SMALL
    W, H, X, LW = cfg["W"], cfg["H"], cfg["IMGX"], cfg["LW"]
    cs = make_case(gpu, dict(SMALL, N=2), bits=8)
    n = 2
    sent = np.full((n, H, W), 0x5A, np.uint8)
    sentUV = np.full((n, H // 2, W), 0x5A, np.uint8)
    ds = DeviceSurfaces(to_dev(gpu, sent, 0), to_dev(gpu, sentUV, 0), None, W, H, 8, True, False)
    er = AMTEraseLogo(ctx, cs["logo"])
    an = AMTAnalyzeLogo(ctx, cs["logo"], 0.35)
    lf = LogoFrame(ctx, [cs["logo"]], 0.35)
    lf.begin(W, H, 8, n)
    d_fades = torch.ones((n, 2), dtype=torch.float32, device=gpu["dev"])
    h_fades = np.ones((n, 2), np.float32)
    rec = torch.zeros((n, 33), dtype=torch.float32, device=gpu["dev"])
    pf, pd, pr = h_fades.ctypes.data_as(C.c_void_p), C.c_void_p(d_fades.data_ptr()), C.c_void_p(rec.data_ptr())

    def desc(**kw):
        d = ds.ref()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    # every entry point through the one reader of the descriptor, in the caller's words
    calls = {
        "[AMTEraseLogo]": (lambda d: lib.amtgpu_erase_surfaces(er.h, d, n, pf), lambda d: lib.amtgpu_erase_surfaces_dfades(er.h, d, n, pd),
                           lambda d: lib.amtgpu_erase_surfaces_dfades_to(er.h, d, d, n, pd)),
        "[AMTAnalyzeLogo]": (lambda d: lib.amtgpu_analyze_surfaces(an.h, d, n, pr),),
        "[LogoFrame]": (lambda d: lib.amtgpu_logoframe_scan_surfaces(lf.h, d, 0, n),),
    }
    for who, fns in calls.items():
        for fn in fns:
            refused(gpu, fn(None), who + " null surface descriptor")
            refused(gpu, fn(C.byref(desc(reserved=1))), who + " reserved field of the surface descriptor must be 0")
            refused(gpu, fn(C.byref(desc(bits=7))), who + " surface bits must be 8..16")
            refused(gpu, fn(C.byref(desc(bits=17))), who + " surface bits must be 8..16")
            refused(gpu, fn(C.byref(desc(msb_aligned=1))), who + " MSB-aligned surfaces are 16-bit containers")
            refused(gpu, fn(C.byref(desc(pitchY=X + LW - 1))), who + " surface pitchY smaller than the rectangle's rows")
    d = desc(pitchUV=X + LW - 1)                                               # interleaved: 2 * (cx + wUV) = X + LW containers
    refused(gpu, lib.amtgpu_erase_surfaces_dfades(er.h, C.byref(d), n, pd), "[AMTEraseLogo] surface pitchUV smaller than the rectangle's rows")
    planar = DeviceSurfaces(ds.Y, to_dev(gpu, sent[:, :H // 2, :W // 2], 0), to_dev(gpu, sent[:, :H // 2, :W // 2], 0), W, H, 8, False, False).ref()
    planar.pitchUV = (X + LW) // 2 - 1
    refused(gpu, lib.amtgpu_erase_surfaces_dfades(er.h, C.byref(planar), n, pd), "[AMTEraseLogo] surface pitchUV smaller than the rectangle's rows")
    # mode != 0
    er1 = AMTEraseLogo(ctx, cs["logo"], "", 1, 16)
    refused(gpu, lib.amtgpu_erase_surfaces_dfades(er1.h, C.byref(desc()), n, pd), "[AMTEraseLogo] only mode 0 is supported")
    # null fades
    refused(gpu, lib.amtgpu_erase_surfaces(er.h, C.byref(desc()), n, None), "[AMTEraseLogo] null fades")
    refused(gpu, lib.amtgpu_erase_surfaces_dfades(er.h, C.byref(desc()), n, None), "[AMTEraseLogo] null device fades")
    refused(gpu, lib.amtgpu_erase_surfaces_dfades_to(er.h, C.byref(desc()), C.byref(desc()), n, None), "[AMTEraseLogo] null device fades")
    # a destination laid out differently
    for kw in (dict(pitchY=W + 2), dict(pitchUV=W + 2), dict(strideY=2 * W * H), dict(strideUV=W * H), dict(interleaved=0, V=ds.U.data_ptr())):
        a, b = desc(), desc(**kw)
        refused(gpu, lib.amtgpu_erase_surfaces_dfades_to(er.h, C.byref(a), C.byref(b), n, pd), "[AMTEraseLogo] destination surfaces differ from the source's")
    refused(gpu, lib.amtgpu_erase_surfaces_dfades_to(er.h, C.byref(desc()), None, n, pd), "[AMTEraseLogo] null surface descriptor")
    # LogoFrame: the depth given to begin()
    lf.begin(W, H, 10, n)
    refused(gpu, lib.amtgpu_logoframe_scan_surfaces(lf.h, C.byref(desc()), 0, n), "[LogoFrame] surface bits differ from the depth given to amtgpu_logoframe_begin")
    # the Python layer's own argument rules
    with pytest.raises(ValueError):
        er.erase_surfaces(ds)
    with pytest.raises(ValueError):
        er.erase_surfaces(ds, fades=h_fades, d_fades=d_fades)
    with pytest.raises(ValueError):
        er.erase_surfaces(ds, fades=h_fades, dst=ds)
    # nothing above touched the surfaces; nframes == 0 returns 1 and touches nothing either (fades {1, 1} would rewrite the rectangle)
    lf.begin(W, H, 8, n)
    assert lib.amtgpu_erase_surfaces(er.h, C.byref(desc()), 0, pf) == 1
    assert lib.amtgpu_erase_surfaces_dfades(er.h, C.byref(desc()), 0, pd) == 1
    assert lib.amtgpu_erase_surfaces_dfades_to(er.h, C.byref(desc()), C.byref(desc()), 0, pd) == 1
    assert lib.amtgpu_analyze_surfaces(an.h, C.byref(desc()), 0, pr) == 1
    assert lib.amtgpu_logoframe_scan_surfaces(lf.h, C.byref(desc()), 0, 0) == 1
    ctx.synchronize()
    assert np.all(host(ds.Y) == 0x5A) and np.all(host(ds.U) == 0x5A) and np.all(rec.cpu().numpy() == 0)
    # ... and the same descriptor with frames is taken
    assert lib.amtgpu_erase_surfaces_dfades(er.h, C.byref(desc()), n, pd) == 1
    ctx.synchronize()
    assert not np.all(host(ds.Y) == 0x5A)
