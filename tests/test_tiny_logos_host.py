"""The tiny-logo cases of tests/tiny_logos.py on the CPU: the case list is what it says (mask pixel counts per regime, field-mode and
in-between fades in every "all" clip), the CPU oracle agrees with the compiled reference on every one of them -- mask tables, scan
scores, analysis records, fades and erased frames, byte for byte, NaN where the reference has NaN -- and the product's host tables are
the oracle's.  This is what entitles tests/test_gpu_tiny_logos.py to take its expected values from the oracle alone.

Sizes the compiled reference itself fails on: none.  It takes every size of the list at every depth and placement."""
import ctypes as C

import numpy as np
import pytest

import tiny_logos as T
from amtlib import Ref, _ptr

needs_ref = pytest.mark.skipif(not Ref.available(), reason="oracle/_ref/libamt_ref.so not built")
CASE_IDS = [T.case_id(c) for c in T.CASES]


def test_case_list_is_what_it_says():
    """mask pixel counts (deinterlaced, top field, bottom field): 0 / 0 / 0 for "none", positive / 0 / 0 for "mixed", positive x 3 for "all";
    every "all" clip has a field-mode fade pair and a pair off {0, 1} in the oracle's CalcFade -- settled here, from the oracle alone"""
    for case in T.CASES:
        group, w, h = case
        for ratio in T.RATIOS:
            counts = T.mask_counts(w, h, ratio)
            print("tiny_logos mask counts %-14s maskratio %.2f  deint %3d  top %3d  bottom %3d" % (T.case_id(case), ratio, *counts))
            if group == "none":
                assert counts == (0, 0, 0), (case, ratio, counts)
            elif group == "mixed":
                assert counts[0] > 0 and counts[1:] == (0, 0), (case, ratio, counts)
            else:
                assert min(counts) > 0, (case, ratio, counts)
    assert T.mask_counts(130, 10, 0.35)[1:] == (126, 126) and T.mask_counts(6, 10, 0.35) == (12, 2, 2)      # one mask row in the field logos
    for (w, h) in T.GROUPS["all"]:
        for bits in T.DEPTHS:
            for ratio in T.RATIOS:
                o = T.oracle_results(w, h, bits, "inside", ratio)
                f = o["fades"]
                assert np.isfinite(o["records"]).all() and np.isfinite(o["scan"]).all()
                assert (f[:, 0] != f[:, 1]).any(), ("no field-mode fade pair", w, h, bits, ratio, f.tolist())
                assert ((f != 0) & (f != 1)).any(), ("no fade off {0, 1}", w, h, bits, ratio, f.tolist())
                # the rectangle's samples are the placement's only input: the corners have the same records
                for placement in T.PLACEMENTS[1:]:
                    p = T.oracle_results(w, h, bits, placement, ratio)
                    assert p["records"].tobytes() == o["records"].tobytes() and p["scan"].tobytes() == o["scan"].tobytes()


def test_records_are_nan_exactly_where_a_logo_has_no_mask_pixel():
    for group, w, h in T.CASES:
        for bits in T.DEPTHS:
            for ratio in T.RATIOS:
                o = T.oracle_results(w, h, bits, "inside", ratio)
                rec = o["records"]
                if group == "none":
                    assert np.isnan(rec).all() and np.isnan(o["scan"]).all()
                elif group == "mixed":
                    assert np.isfinite(rec[:, :11]).all() and np.isnan(rec[:, 11:]).all() and np.isfinite(o["scan"]).all()
                else:
                    assert np.isfinite(rec).all() and np.isfinite(o["scan"]).all()


def test_opacities_and_depth_of_the_clips():
    """noise over the whole depth, fields that differ in frames 3 and 7, the same rectangle at every placement"""
    for bits in T.DEPTHS:
        maxv = (1 << bits) - 1
        clip = T.tiny_clip(130, 10, bits, "inside")
        assert int(clip["Y"].max()) > 0.99 * maxv and int(clip["Y"].min()) < 0.01 * maxv and clip["Y"].shape == (9, 240, 384)
        rY = T.rect_samples(130, 10, bits)[0]
        for placement in T.PLACEMENTS:
            W, H, X, Y0, pad = T.geometry(130, 10, placement)
            c = T.tiny_clip(130, 10, bits, placement)
            assert np.array_equal(c["Y"][:, Y0:Y0 + 10, X:X + 130], rY) and c["Y"].shape == (9, H, W + pad)
    assert T.geometry(10, 10, "bottom_right") == (32, 16, 22, 6, 0) and T.geometry(130, 10, "bottom_right") == (160, 16, 30, 6, 0)


def test_guarded_clip_layout():
    clip = T.tiny_clip(6, 10, 10, "bottom_right")
    g = T.GuardedClip(clip, 0xFFFF)
    assert g.size == 4 * T.GUARD + 9 * (32 * 16 + 2 * 16 * 8) and g.flat.dtype == np.uint16
    for k in "YUV":
        assert np.array_equal(g.plane(k), clip[k])
    assert g.guards_intact(g.flat) and g.spans[0] == (0, T.GUARD) and g.spans[-1][1] == g.size
    assert g.off["Y"] == T.GUARD and g.off["U"] == 2 * T.GUARD + 9 * 32 * 16
    for a, b in g.spans:
        assert b - a >= 64 * 1024
        flat = g.flat.copy()
        flat[b - 1] ^= 1
        assert not g.guards_intact(flat)


# ---- the oracle against the compiled reference -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref():
    return Ref()


def saved_logo(tmp_path, w, h, placement):
    lo = T.oracle_logo(w, h, placement)
    path = str(tmp_path / ("%dx%d_%s.lgd" % (w, h, placement))).encode()
    assert T.oracle().lib.orc_logo_save(lo, path, b"tiny", 7) == 1
    return lo, path


@needs_ref
@pytest.mark.parametrize("case", T.CASES, ids=CASE_IDS)
def test_oracle_mask_tables_are_the_references(ref, tmp_path, case):
    """count, positions (the mask), kernels, scales and blackScore of the three evaluation logos at both mask ratios"""
    _, w, h = case
    orc = T.oracle()
    lo, path = saved_logo(tmp_path, w, h, "inside")
    rh = ref.lib.ref_logo_load(path)
    assert rh, ref.lib.ref_last_error()
    assert np.array_equal(ref.logo_data(rh), T.tiny_logo(w, h))
    for ratio in T.RATIOS:
        for kind in range(3):
            o2, r2 = (orc.lib.orc_logo_deint(lo), ref.lib.ref_logo_deint(rh)) if kind == 0 else (orc.lib.orc_logo_field(lo, kind - 1), ref.lib.ref_logo_field(rh, kind - 1))
            orc.lib.orc_logo_create_mask(o2, ratio, 1)
            ref.lib.ref_logo_create_mask(r2, ratio)
            oi, ri = orc.logo_info(o2), ref.logo_info(r2)
            assert list(oi[:9]) == list(ri[:9]), (kind, ratio)
            data, mask, ker, sc, black, mp, cnt = orc.logo_arrays(o2)
            assert cnt <= mp <= oi[0] * oi[1]                      # (maskpixels counts the border's pixels too, `count` only those with a window)
            if mp == 0:                                           # the 2 x 1 field logos of 2 x 2 at maskratio 0.35: (int)(2 * 0.35) pixels
                assert (w, h, ratio) == (2, 2, 0.35) and kind > 0 and ri[8] == 0
                assert T.same_bytes_or_nan([orc.lib.orc_logo_black_score(o2)], [ref.lib.ref_logo_black_score(r2)])
                continue
            rmask, rker, rsc, rblack, rmp = ref.logo_tables(r2, cnt)
            assert np.array_equal(data[:2 * oi[0] * oi[1]], ref.logo_data(r2)[:2 * oi[0] * oi[1]])
            assert rmp == mp and np.array_equal(mask, rmask)
            assert ker[:cnt * 25].tobytes() == rker.tobytes() and sc[:cnt * 64].tobytes() == rsc.tobytes()
            assert T.same_bytes_or_nan([black], [rblack]), (kind, ratio, black, rblack)
            assert (cnt == 0) == (rblack == 0)                    # no pixel to add up: blackScore 0, every record 0 / 0
    ref.lib.ref_logo_free(rh)


@needs_ref
@pytest.mark.parametrize("placement", T.PLACEMENTS)
@pytest.mark.parametrize("case", T.CASES, ids=CASE_IDS)
def test_oracle_scan_scores_are_the_references(ref, tmp_path, case, placement):
    """LogoFrame::scanFrames.  8 bits: at every placement.  Deeper clips: ScanFrame<uint16_t> multiplies the byte pitch into a uint16_t
    pointer (LogoScan.hpp:1547, 1561-1562), so the reference reads rectangle row y at frame row 2 (imgy + y); called with a doubled
    pitch the oracle addresses what the reference does, which fits the frame only at "inside" (tests/test_oracle_vs_ref.py)."""
    _, w, h = case
    W, H, X, Y0, _ = T.geometry(w, h, placement)
    lo, path = saved_logo(tmp_path, w, h, placement)
    for bits in T.DEPTHS if placement == "inside" else (8,):
        Y = np.ascontiguousarray(T.tiny_clip(w, h, bits, placement)["Y"][:, :, :W])
        for ratio in T.RATIOS:
            ev_r = np.zeros(T.N_FRAMES * 2, np.float32)
            best, share = C.c_int(), C.c_float()
            text = C.create_string_buffer(1 << 16)
            ok = ref.lib.ref_logoframe((C.c_char_p * 1)(path), 1, ratio, _ptr(Y), Y.strides[0], W, bits, W, H, T.N_FRAMES, 30000, 1001, _ptr(ev_r), -1,
                                       C.byref(best), C.byref(share), 0, str(tmp_path / "lf.txt").encode(), text, len(text))
            assert ok == 1, ref.lib.ref_last_error()
            d = T.oracle().lib.orc_logo_deint(lo)
            T.oracle().lib.orc_logo_create_mask(d, ratio, 1)
            if bits == 8:
                want = T.oracle_results(w, h, bits, placement, ratio)["scan"]
            else:
                assert 2 * (Y0 + h) <= H and (W * 2) % 64 == 0
                ev_o = np.zeros(T.N_FRAMES * 2, np.float32)
                T.oracle().lib.orc_logoframe_scan((C.c_void_p * 1)(d), 1, _ptr(Y), Y.strides[0], 2 * W, bits, W, H, T.N_FRAMES, _ptr(ev_o))
                want = ev_o
            T.assert_records(want, ev_r, "scan %s %d bits maskratio %s" % (placement, bits, ratio))
            assert np.isnan(ev_r).all() == (case[0] == "none")


@needs_ref
@pytest.mark.parametrize("placement", T.PLACEMENTS)
@pytest.mark.parametrize("case", T.CASES, ids=CASE_IDS)
def test_oracle_records_fades_and_erased_frames_are_the_references(ref, tmp_path, case, placement):
    """AMTAnalyzeLogo's 33 floats per frame, AMTEraseLogo::CalcFade and the erased planes, at 8, 10 and 16 bits"""
    _, w, h = case
    W, H, X, Y0, _ = T.geometry(w, h, placement)
    lo, path = saved_logo(tmp_path, w, h, placement)
    n = T.N_FRAMES
    for bits in T.DEPTHS:
        clip = T.tiny_clip(w, h, bits, placement)
        for ratio in T.RATIOS:
            o = T.oracle_results(w, h, bits, placement, ratio)
            Y, U, V = (np.array(clip[k], copy=True) for k in "YUV")
            an_r = np.zeros(n * 33, np.float32)
            assert ref.lib.ref_analyze(path, ratio, _ptr(Y), _ptr(U), _ptr(V), Y.strides[0], U.strides[0], Y.shape[2], U.shape[2], bits, W, H, n,
                                       _ptr(an_r)) == 1, ref.lib.ref_last_error()
            T.assert_records(o["records"], an_r, "records %s %d bits maskratio %s" % (placement, bits, ratio))
            fades_r = np.zeros(n * 2, np.float32)
            assert ref.lib.ref_erase(path, b"", 16, ratio, _ptr(Y), _ptr(U), _ptr(V), Y.strides[0], U.strides[0], Y.shape[2], U.shape[2], bits, W, H, n,
                                     _ptr(fades_r)) == 1, ref.lib.ref_last_error()
            assert o["fades"].tobytes() == fades_r.tobytes(), (bits, ratio, o["fades"].tolist(), fades_r.tolist())
            for k, got in zip("YUV", (Y, U, V)):
                assert np.array_equal(got, o["erased"][k]), (k, bits, ratio)
            if case[0] == "none":
                assert not fades_r.any() and np.array_equal(Y, clip["Y"])     # argmin of eleven NaNs is 0: nothing is erased
            else:
                assert not np.array_equal(Y, clip["Y"])


# ---- the product's host tables against the oracle's ------------------------------------------------------------------------------------
class HostContext:
    """what Logo needs of a Context, without a device: the library and a null handle (tests/test_abi_and_host.py calls it the same way)"""

    def __init__(self):
        from amatsukaze_amd import build as b
        b.build()
        from amatsukaze_amd import binding
        self.lib, self.h = binding.load(), None

    def check(self, ok, what=""):
        assert ok, what


@pytest.fixture(scope="module")
def host_ctx():
    return HostContext()


@pytest.mark.parametrize("case", T.CASES, ids=CASE_IDS)
def test_product_host_tables_are_the_oracles(host_ctx, tmp_path, case):
    """Logo.from_planes and amtgpu_logo_load of the oracle's file, then amtgpu_logo_mask_tables of the three evaluation logos at both
    mask ratios: maskpixels, count, mask, kernels, scales, blackScore"""
    from amatsukaze_amd import Logo
    _, w, h = case
    W, H, X, Y0, _ = T.geometry(w, h, "inside")
    orc = T.oracle()
    data = T.tiny_logo(w, h)
    lo, path = saved_logo(tmp_path, w, h, "inside")
    made = Logo.from_planes(host_ctx, data, w, h, W, H, X, Y0)
    loaded = Logo.load(host_ctx, path.decode())
    out = tmp_path / "product.lgd"
    made.save(out, "tiny", 7)
    assert out.read_bytes() == open(path, "rb").read()
    for logo in (made, loaded):
        assert logo.info == dict(w=w, h=h, logUVx=1, logUVy=1, imgw=W, imgh=H, imgx=X, imgy=Y0) and logo.planes.tobytes() == data.tobytes()
        for ratio in T.RATIOS:
            for kind in range(3):
                o2 = orc.lib.orc_logo_deint(lo) if kind == 0 else orc.lib.orc_logo_field(lo, kind - 1)
                orc.lib.orc_logo_create_mask(o2, ratio, 1)
                _, mask, ker, sc, black, mp, cnt = orc.logo_arrays(o2)
                t = logo.mask_tables(kind, ratio)
                assert (t["maskpixels"], t["count"]) == (mp, cnt), (kind, ratio)
                if mp == 0:                                       # (logo_arrays hands out no tables then: 2 x 1 field logos at 0.35)
                    assert not t["mask"].any() and t["kernels"].size == 0 and T.same_bytes_or_nan([t["blackScore"]], [orc.lib.orc_logo_black_score(o2)])
                    continue
                assert np.array_equal(t["mask"], mask)
                assert t["kernels"].tobytes() == ker[:cnt * 25].tobytes() and t["scales"].tobytes() == sc[:cnt * 64].tobytes()
                assert T.same_bytes_or_nan([t["blackScore"]], [black]), (kind, ratio, t["blackScore"], black)
