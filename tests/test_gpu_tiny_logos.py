"""The logo kernels on the smallest logos each kernel form takes (tests/tiny_logos.py: the "none", "mixed" and "all" regimes around
w >= 6, h >= 5 and count > 0 of eval_engine.hip pair_eligible / tiles_usable), against the CPU oracle, which tests/test_tiny_logos_host.py
holds against the compiled reference on every one of these cases.

The rule for records: identical bytes wherever the oracle's value is not NaN, NaN (any payload) wherever it is.

Placement "inside" puts the rectangle at (224, 18) of a padded 352 x 240 frame; the corner placements put it flush into the first and
the last samples of unpadded planes that lie in ONE allocation between guard containers (tiny_logos.GuardedClip): everything runs twice
there, over guards of zeros and of ones -- a kernel that reads a guard gives two answers, one that writes a guard leaves a trace."""
import functools

import numpy as np
import pytest

import linear_terms_ref as R
import surface_clips as SC
import surface_erase_ref as ER
import test_gpu_erase_shapes as ES
import test_gpu_surface_erase as SE
import tiny_logos as T
from test_gpu_parity import gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

CASE_IDS = [T.case_id(c) for c in T.CASES]
CORNERS = T.PLACEMENTS[1:]
ALL_MODES = ("exact", "linear_unguarded", "linear", "monitored")
ERASE_SIZES = ((2, 2), (4, 4), (6, 6), (10, 10))


# ---- device side ---------------------------------------------------------------------------------------------------------------------
def as_tensor(gpu, a):
    a = np.array(a, copy=True, order="C")                 # (the helper's clips are shared and read-only)
    return gpu["torch"].from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)).to(gpu["dev"])


def device_clip(gpu, w, h, bits, placement="inside"):
    from amatsukaze_amd import DeviceClip
    W, H = T.geometry(w, h, placement)[:2]
    clip = T.tiny_clip(w, h, bits, placement)
    return DeviceClip(*(as_tensor(gpu, clip[k]) for k in "YUV"), width=W, height=H, bits=bits)


def guarded_device_clip(gpu, w, h, bits, placement, ones, clip=None):
    """(DeviceClip whose planes are views into one flat device buffer, that buffer, its host layout)"""
    from amatsukaze_amd import DeviceClip
    torch = gpu["torch"]
    W, H = T.geometry(w, h, placement)[:2]
    fill = (0xFF if bits <= 8 else 0xFFFF) if ones else 0
    g = T.GuardedClip(T.tiny_clip(w, h, bits, placement) if clip is None else clip, fill)
    flat = as_tensor(gpu, g.flat)
    views = [torch.as_strided(flat, g.shapes[k], (g.shapes[k][1] * g.shapes[k][2], g.shapes[k][2], 1), g.off[k]) for k in "YUV"]
    return DeviceClip(*views, width=W, height=H, bits=bits), flat, g


def host_flat(g, flat):
    return flat.cpu().numpy().view(g.dt)


def product_logo(gpu, w, h, placement="inside", xy=None):
    from amatsukaze_amd import Logo
    W, H, X, Y0, _ = T.geometry(w, h, placement)
    if xy is not None:
        X, Y0 = xy
    return Logo.from_planes(gpu["ctx"], T.tiny_logo(w, h), w, h, W, H, X, Y0)


def profiled(gpu, fn):
    """(fn(), names of the kernels that ran)"""
    ctx = gpu["ctx"]
    ctx.profile(True)
    try:
        out = fn()
        used = sorted(k for k, (calls, _) in ctx.profile_report().items() if calls)
    finally:
        ctx.profile(False)
    return out, used


def is_tile_kernel(name):
    return name.startswith("logo_eval_pair") or name.startswith("logo_eval_linear_kernel")


def scan(gpu, logos, ratio, dclip):
    from amatsukaze_amd import LogoFrame
    lf = LogoFrame(gpu["ctx"], logos, ratio)
    lf.scanFrames(dclip)
    return lf.evalResults


def analyze(gpu, logo, ratio, mode, dclip):
    from amatsukaze_amd import AMTAnalyzeLogo
    return AMTAnalyzeLogo(gpu["ctx"], logo, ratio, mode=mode).analyze(dclip)


@functools.lru_cache(maxsize=None)
def frames_ref(w, h, bits, ratio):
    """tests/linear_terms_ref.py on the case's "inside" clip: the oracle's records stated twice, `own` and tol = K * own"""
    W, H, X, Y0, _ = T.geometry(w, h, "inside")
    Y = np.ascontiguousarray(T.tiny_clip(w, h, bits, "inside")["Y"])
    ref = R.FramesRef("tiny %dx%d, %d bits, maskratio %s" % (w, h, bits, ratio), T.tiny_logo(w, h), (w, h, X, Y0, H), ratio, bits, Y, W=W, mutants=False)
    assert ref.want.tobytes() == T.oracle_results(w, h, bits, "inside", ratio)["records"].tobytes()
    return ref


def check_linear_records(gpu, an, got, w, h, bits, ratio, what):
    """the unguarded linear kernel's records of an "all" case: within K x the oracle's own rounding (FramesRef.check); should `own` be 0 --
    the fp32 and the float64 statement agree to the last bit, which two mask pixels can do -- within the library's own bound instead.
    (What this check found: 8 x 10 at 16 bits, maskratio 0.35, frame 3, deinterlaced logo, fade 0.6 came out 0.448242873 against the
    oracle's 0.44828701 -- 4.4e-5 off at tol 5.8e-6 -- while the host summed the taps that multiply the window mean in fp32; with the sum
    formed in double, EvalEngine::ensure_tiles, the case's largest error is 2.6e-6.)"""
    ref = frames_ref(w, h, bits, ratio)
    want = ref.want
    if ref.own > 0:
        err = ref.check(got, what)
        print("tiny_logos linear %s: rule K * own, own %.3e, tol %.3e, max error %.3e" % (what, ref.own, ref.tol, err))
        return
    counts = T.mask_counts(w, h, ratio)
    assert min(counts) <= 2, (what, "own == 0 with more than two mask pixels in every logo", counts)
    scale = max(1.0, float(np.abs(want).max()))
    for k in range(3):
        err = float(np.abs(got.astype(np.float64) - want)[:, 11 * k:11 * k + 11].max())
        bound = an.error_bound(k, bits) * scale
        print("tiny_logos linear %s: rule error_bound (own == 0), logo %d, bound %.3e, max error %.3e" % (what, k, bound, err))
        assert err <= bound, (what, k, err, bound)


# ---- scan ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", T.DEPTHS)
@pytest.mark.parametrize("ratio", T.RATIOS)
@pytest.mark.parametrize("case", T.CASES, ids=CASE_IDS)
def test_scan_one_logo(gpu, case, ratio, bits):
    group, w, h = case
    got, used = profiled(gpu, lambda: scan(gpu, [product_logo(gpu, w, h)], ratio, device_clip(gpu, w, h, bits)))
    if group == "none":
        assert used and not any(is_tile_kernel(k) for k in used), used
    else:
        assert used == ["logo_eval_pair_kernel.scan"], used
    T.assert_records(got[:, 0], T.oracle_results(w, h, bits, "inside", ratio)["scan"], "scan of %s" % T.case_id(case))


# (first logo: its own "inside" clip and place; second logo: elsewhere in the same frame, over plain noise)
TWO_LOGOS = {"6x6+10x10": ((6, 6), (10, 10), (100, 40), True), "130x10+6x10": ((130, 10), (6, 10), (30, 200), True),
             "8x10+6x8": ((8, 10), (6, 8), (346, 232), True), "10x10+2x2": ((10, 10), (2, 2), (2, 0), False), "4x10+6x6": ((4, 10), (6, 6), (60, 100), False)}


@pytest.mark.parametrize("bits", T.DEPTHS)
@pytest.mark.parametrize("ratio", T.RATIOS)
@pytest.mark.parametrize("pair", sorted(TWO_LOGOS))
def test_scan_two_logos_of_different_sizes(gpu, pair, ratio, bits):
    """one engine, two tiny logos: the pair kernel when both have mask pixels; a logo without any keeps the whole engine off the tiles"""
    (w1, h1), (w2, h2), xy2, tiles = TWO_LOGOS[pair]
    W, H = T.geometry(w1, h1, "inside")[:2]
    logos = [product_logo(gpu, w1, h1), product_logo(gpu, w2, h2, xy=xy2)]
    got, used = profiled(gpu, lambda: scan(gpu, logos, ratio, device_clip(gpu, w1, h1, bits)))
    assert (used == ["logo_eval_pair_kernel.scan"]) if tiles else (used and not any(is_tile_kernel(k) for k in used)), used
    orc = T.oracle()
    hs = []
    for lo in (T.oracle_logo(w1, h1, "inside"), orc.make_logo(T.tiny_logo(w2, h2), w2, h2, W, H, *xy2)):
        d = orc.lib.orc_logo_deint(lo)
        orc.lib.orc_logo_create_mask(d, ratio, 1)
        hs.append(d)
    want = T.oracle_scan(hs, T.tiny_clip(w1, h1, bits, "inside")["Y"], bits, W, H)
    assert want[:, 0].tobytes() == T.oracle_results(w1, h1, bits, "inside", ratio)["scan"].tobytes()
    T.assert_records(got, want, "scan of " + pair)


# ---- analysis --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", T.DEPTHS)
@pytest.mark.parametrize("ratio", T.RATIOS)
@pytest.mark.parametrize("case", T.CASES, ids=CASE_IDS)
def test_exact_analysis(gpu, case, ratio, bits):
    group, w, h = case
    got, used = profiled(gpu, lambda: analyze(gpu, product_logo(gpu, w, h), ratio, "exact", device_clip(gpu, w, h, bits)))
    assert used == ["logo_eval_fused_kernel.analysis"], used
    T.assert_records(got, T.oracle_results(w, h, bits, "inside", ratio)["records"], "exact analysis of %s" % T.case_id(case))


@pytest.mark.parametrize("bits", T.DEPTHS)
@pytest.mark.parametrize("ratio", T.RATIOS)
@pytest.mark.parametrize("case", T.CASES, ids=CASE_IDS)
def test_linear_analysis_modes(gpu, case, ratio, bits):
    from amatsukaze_amd import AMTAnalyzeLogo, AMTEraseLogo
    group, w, h = case
    logo, dclip = product_logo(gpu, w, h), device_clip(gpu, w, h, bits)
    want = T.oracle_results(w, h, bits, "inside", ratio)
    what = "%s, %d bits, maskratio %s" % (T.case_id(case), bits, ratio)
    for mode in ALL_MODES[1:]:
        an = AMTAnalyzeLogo(gpu["ctx"], logo, ratio, mode=mode)
        got, used = profiled(gpu, lambda: an.analyze(dclip))
        assert got.shape == (T.N_FRAMES, 33)
        if group != "all":
            # a logo of the engine is below the tile kernels' limits: the exact kernel's records, whatever the mode
            assert not any(is_tile_kernel(k) for k in used) and any(k.startswith("logo_eval_fused_kernel") for k in used), (mode, used)
            T.assert_records(got, want["records"], mode + " analysis of " + what)
            continue
        assert any(k.startswith("logo_eval_linear_kernel") for k in used), (mode, used)
        if mode == "linear_unguarded":
            assert not any("fused" in k for k in used), used
            check_linear_records(gpu, an, got, w, h, bits, ratio, what)
        else:
            er = AMTEraseLogo(gpu["ctx"], logo, "", 0, 16)
            fades = er.calc_fades(got, T.N_FRAMES)
            assert fades.tobytes() == er.calc_fades(want["records"], T.N_FRAMES).tobytes() == want["fades"].tobytes(), (mode, what)


# ---- erase -----------------------------------------------------------------------------------------------------------------------------
def erase_geom(w, h):
    W, H, X, Y0, pad = T.geometry(w, h, "inside")
    return (W, H, w, h, X, Y0, pad, pad // 2, 0)


def build_erase(gpu, w, h, bits, n):
    """test_gpu_erase_shapes.build on the tiny logo.  One case it cannot take: its check that the oracle changed every plane fails for
    2 x 2 with one frame, whose only fade pair is a field-mode one -- the 1 x 1 chroma plane then stays, which is the point of the case;
    that one is built here from the same parts, with the check on the luma alone."""
    data = T.tiny_logo(w, h)
    if (w, h, n) != (2, 2, 1):
        return ES.build(gpu, erase_geom(w, h), bits, n, data=data)
    from amatsukaze_amd import AMTEraseLogo, Logo
    W, H, LW, LH, X, Y0, padY, padUV, off = erase_geom(w, h)
    planes = ES.make_planes(np.random.RandomState(1000 * bits + n), n, W, H, W + padY, W // 2 + padUV, bits, (X, Y0, LW, LH))
    fades = ES.fades_for(n)
    ES.assert_finite_mix(data, LW, LH, planes, (X, Y0), fades, (1 << bits) - 1)
    logo = Logo.from_planes(gpu["ctx"], data, LW, LH, W, H, X, Y0)
    want = T.oracle_erase(T.oracle().make_logo(data, LW, LH, W, H, X, Y0), planes, bits, fades)
    assert not np.array_equal(want["Y"], planes["Y"])
    return dict(W=W, H=H, rect=(X, Y0, LW, LH), off=off, bits=bits, planes=planes, want=want, fades=fades, er=AMTEraseLogo(gpu["ctx"], logo), logo=logo)


@pytest.mark.parametrize("n", [27, 1])
@pytest.mark.parametrize("bits", T.DEPTHS)
@pytest.mark.parametrize("size", ERASE_SIZES, ids=lambda s: "%dx%d" % s)
def test_erase_whole_planes(gpu, size, bits, n):
    w, h = size
    cs = build_erase(gpu, w, h, bits, n)
    assert cs["er"].rect == (*T.geometry(w, h, "inside")[2:4], w, h, 1)
    field = cs["fades"][:, 0] != cs["fades"][:, 1]
    assert field.any()
    if (w, h) == (2, 2):
        # the 1 x 1 chroma plane's only row is an odd last row: field-mode frames leave both chroma samples as they were
        X, Y0 = cs["rect"][:2]
        for k in "UV":
            assert np.array_equal(cs["want"][k][field], cs["planes"][k][field])
            if n > 1:
                assert (cs["want"][k][~field, Y0 // 2, X // 2] != cs["planes"][k][~field, Y0 // 2, X // 2]).any()
    ES.run_both_entries(gpu, cs)


@pytest.mark.parametrize("n", [27, 1])
@pytest.mark.parametrize("layout", [(8, 1, 0), (10, 1, 1)], ids=["NV12", "P010"])
@pytest.mark.parametrize("size", ERASE_SIZES, ids=lambda s: "%dx%d" % s)
def test_erase_decoder_surfaces(gpu, size, layout, n):
    """test_gpu_surface_erase's build / run_both_entries on the tiny logos (2 x 2 with one frame as in build_erase)"""
    from amatsukaze_amd import AMTEraseLogo, Logo
    w, h = size
    bits, il, msb = layout
    data, geom, orc = T.tiny_logo(w, h), erase_geom(w, h), T.oracle()
    if (w, h, n) != (2, 2, 1):
        cs = SE.build(gpu, orc, geom, layout, n, data=data)
    else:
        W, H, LW, LH, X, Y0, padY, padUV, off = geom
        planes = ES.make_planes(np.random.RandomState(1000 * bits + n), n, W, H, W, W // 2, bits, (X, Y0, LW, LH))
        if msb:
            planes = {k: np.minimum(v, (1 << bits) - 1).astype(v.dtype) for k, v in planes.items()}
        fades = ES.fades_for(n)
        ES.assert_finite_mix(data, LW, LH, planes, (X, Y0), fades, (1 << bits) - 1)
        surf = SC.to_surfaces(planes, bits, il, msb, np.random.default_rng(bits), padY, padUV, SE.fill_of(bits))
        er = AMTEraseLogo(gpu["ctx"], Logo.from_planes(gpu["ctx"], data, LW, LH, W, H, X, Y0))
        want = ER.expected_surfaces(orc, orc.make_logo(data, LW, LH, W, H, X, Y0), surf, W, H, bits, il, msb, (X, Y0, LW, LH), fades, er.rect[4])
        assert not np.array_equal(want["Y"], surf["Y"]) and np.array_equal(want["U"], surf["U"])      # field mode: the chroma pair stays
        cs = dict(W=W, H=H, layout=layout, off=off, surf=surf, want=want, fades=fades, er=er)
    SE.run_both_entries(gpu, cs)


@pytest.mark.parametrize("odd_pitch", [False, True])
@pytest.mark.parametrize("bits", T.DEPTHS)
@pytest.mark.parametrize("size", [(2, 2), (6, 6)], ids=lambda s: "%dx%d" % s)
def test_erase_rect_on_bare_rectangles(gpu, size, bits, odd_pitch):
    """erase_rect on planes that hold only the rectangle, contiguous (chroma rows of 1 and 3 samples: an odd pitch by themselves) and with
    odd luma and chroma pitches; expected samples from the whole-plane case"""
    w, h = size
    cs = build_erase(gpu, w, h, bits, 27)
    X, Y0 = cs["rect"][:2]
    rng = np.random.RandomState(bits)
    pads = (1, 2) if odd_pitch else (0, 0)
    dev, want = {}, {}
    for k, (px, py, pw, ph, pad) in (("Y", (X, Y0, w, h, pads[0])), ("U", (X // 2, Y0 // 2, w // 2, h // 2, pads[1])), ("V", (X // 2, Y0 // 2, w // 2, h // 2, pads[1]))):
        a = rng.randint(0, (1 << bits), (27, ph, pw + pad)).astype(cs["planes"][k].dtype)
        e = a.copy()
        a[:, :, :pw] = cs["planes"][k][:, py:py + ph, px:px + pw]
        e[:, :, :pw] = cs["want"][k][:, py:py + ph, px:px + pw]
        dev[k], want[k] = ES.to_dev(gpu, a, 0), e
    assert (int(dev["Y"].stride(1)) % 2 == 1) == odd_pitch and int(dev["U"].stride(1)) % 2 == 1
    cs["er"].erase_rect(dev["Y"], dev["U"], dev["V"], bits, cs["fades"])
    gpu["ctx"].synchronize()
    for k in "YUV":
        got = ES.host(dev[k])
        assert np.array_equal(got, want[k]), (k, [int(v[0]) for v in np.nonzero(got != want[k])])


# ---- the chain -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", T.DEPTHS)
@pytest.mark.parametrize("size", [(6, 10), (10, 10)], ids=lambda s: "%dx%d" % s)
def test_chain_without_a_synchronise(gpu, size, bits):
    """analyze -> calc_fades_device -> erase_device_fades, stream-ordered: the host-decided path's fades and frames, which are the oracle's"""
    from amatsukaze_amd import AMTAnalyzeLogo, AMTEraseLogo
    torch = gpu["torch"]
    w, h = size
    logo = product_logo(gpu, w, h)
    want = T.oracle_results(w, h, bits, "inside", 0.35)
    an = AMTAnalyzeLogo(gpu["ctx"], logo, 0.35)
    er = AMTEraseLogo(gpu["ctx"], logo, "", 0, 16)
    host_clip = device_clip(gpu, w, h, bits)
    fades = er.calc_fades(an.analyze(host_clip), T.N_FRAMES)
    er.erase(host_clip, fades)
    dc = device_clip(gpu, w, h, bits)
    d_rec = torch.empty((T.N_FRAMES, 33), dtype=torch.float32, device=gpu["dev"])
    an.analyze_device(dc.Y, bits, d_rec)
    d_f = er.calc_fades_device(d_rec, T.N_FRAMES)
    er.erase_device_fades(dc, d_f)
    gpu["ctx"].synchronize()
    assert d_f.cpu().numpy().tobytes() == fades.tobytes() == want["fades"].tobytes()
    for k in "YUV":
        assert torch.equal(getattr(dc, k), getattr(host_clip, k)), k
        assert np.array_equal(ES.host(getattr(dc, k)), want["erased"][k]), k
    assert np.abs(fades).sum() > 0 and not np.array_equal(want["erased"]["Y"], T.tiny_clip(w, h, bits, "inside")["Y"])


# ---- placement (b): flush in the corners of unpadded planes, between guards ------------------------------------------------------------
@pytest.mark.parametrize("bits", T.DEPTHS)
@pytest.mark.parametrize("ratio", T.RATIOS)
@pytest.mark.parametrize("corner", CORNERS)
@pytest.mark.parametrize("case", T.CASES, ids=CASE_IDS)
def test_corner_scan_and_analysis_do_not_depend_on_the_guards(gpu, case, corner, ratio, bits):
    from amatsukaze_amd import AMTAnalyzeLogo
    group, w, h = case
    logo = product_logo(gpu, w, h, corner)
    want = T.oracle_results(w, h, bits, corner, ratio)
    what = "%s in the %s corner, %d bits, maskratio %s" % (T.case_id(case), corner, bits, ratio)
    runs = []
    for ones in (False, True):
        dclip, flat, g = guarded_device_clip(gpu, w, h, bits, corner, ones)
        assert dclip.pitchY == dclip.width and dclip.pitchUV == dclip.width // 2
        out = {"scan": scan(gpu, [logo], ratio, dclip)[:, 0]}
        ans = {mode: AMTAnalyzeLogo(gpu["ctx"], logo, ratio, mode=mode) for mode in ALL_MODES}
        for mode in ALL_MODES:
            out[mode] = ans[mode].analyze(dclip)
        gpu["ctx"].synchronize()
        assert np.array_equal(host_flat(g, flat), g.flat), what + ": a read-only pass wrote to the clip's allocation"
        runs.append(out)
    T.assert_records(runs[0]["scan"], want["scan"], "scan of " + what)
    T.assert_records(runs[0]["exact"], want["records"], "exact analysis of " + what)
    for key in runs[0]:
        assert T.same_bytes_or_nan(runs[1][key], runs[0][key]) and T.same_bytes_or_nan(runs[0][key], runs[1][key]), (key, what, "guards of zeros and of ones give different records")
    for mode in ALL_MODES[1:]:
        if group != "all":
            T.assert_records(runs[0][mode], want["records"], mode + " analysis of " + what)
        elif mode == "linear_unguarded":
            check_linear_records(gpu, ans[mode], runs[0][mode], w, h, bits, ratio, what)     # (the rectangle's samples, hence the records, are the "inside" clip's)
        else:
            assert T.oracle_fades(runs[0][mode]).tobytes() == want["fades"].tobytes(), (mode, what)


@pytest.mark.parametrize("bits", T.DEPTHS)
@pytest.mark.parametrize("corner", CORNERS)
@pytest.mark.parametrize("case", T.CASES, ids=CASE_IDS)
def test_corner_erase_leaves_the_guards(gpu, case, corner, bits):
    """Delogo with the oracle's fades of the clip (all {0, 0} for "none": nothing to rewrite) and with test_gpu_erase_shapes' 9 fade pairs,
    through erase_device_fades into a second guarded clip and in place: the oracle's planes, every guard container as it was"""
    from amatsukaze_amd import AMTEraseLogo
    group, w, h = case
    torch = gpu["torch"]
    er = AMTEraseLogo(gpu["ctx"], product_logo(gpu, w, h, corner))
    clip = T.tiny_clip(w, h, bits, corner)
    lo = T.oracle_logo(w, h, corner)
    for which, fades in (("the clip's own fades", T.oracle_results(w, h, bits, corner, 0.35)["fades"]), ("nine fade pairs", ES.fades_for(9))):
        want = T.oracle_erase(lo, clip, bits, fades)
        assert (group == "none" and which.startswith("the clip")) or not np.array_equal(want["Y"], clip["Y"])
        for ones in (False, True):
            src, sflat, g = guarded_device_clip(gpu, w, h, bits, corner, ones)
            dst, dflat, _ = guarded_device_clip(gpu, w, h, bits, corner, ones)
            er.erase_device_fades(src, torch.from_numpy(np.array(fades, np.float32, copy=True)).to(gpu["dev"]), dst=dst)
            gpu["ctx"].synchronize()
            expect = g.flat.copy()
            for k in "YUV":
                g.plane(k, expect)[...] = want[k]
            what = "%s in the %s corner, %d bits, %s, guards of %s" % (T.case_id(case), corner, bits, which, "ones" if ones else "zeros")
            assert np.array_equal(host_flat(g, dflat), expect) and g.guards_intact(host_flat(g, dflat)), what + ": erase_device_fades(dst)"
            assert np.array_equal(host_flat(g, sflat), g.flat), what + ": the source changed"
            er.erase(src, fades)
            gpu["ctx"].synchronize()
            assert np.array_equal(host_flat(g, sflat), expect) and g.guards_intact(host_flat(g, sflat)), what + ": erase in place"
