"""CPU statement of LogoAnalyzer::ScanLogo (LogoScan.hpp:917-1079) for clips of 8..12 bits, for the tests.

The oracle's own ScanLogo (orc_scanlogo_mt) is 8-bit like the reference's, whose limit comes from its work-file codec (:813), not from
its arithmetic: LogoScan::AddFrame is a template over pixel_t, EvaluateLogo / Normalize / GetLogo take maxv.  This module composes the
whole procedure from pieces that are pinned elsewhere, with maxv = (1 << bits) - 1 wherever the 8-bit text says 255:
  * round 0 and both re-accumulations: scan_ref.ScanAccumulator (numpy AddFrame, pinned by test_scan_ref_host.py);
  * Normalize + GetAB + GetLogo(clean) (:336-342, 367-395, 490-566): restated below in float64 from the int64 sums;
  * the 20 evaluations per kept frame: the oracle's orc_logo_deint, orc_logo_create_mask(0.1), orc_deint_y_u8 / _u16, orc_evaluate_logo.
tests/test_scanlogo_ref_host.py pins the composition at 8 bits against orc_scanlogo_mt byte for byte."""
import ctypes as C

import numpy as np

from amtlib import _ptr
from scan_ref import ScanAccumulator


def _approxim_line(n, sx, sy, sx2, sxy):
    t = n * sx2 - sx * sx
    return (n * sxy - sx * sy) / t, (sx2 * sy - sx * sxy) / t


def _calc_dist(a, b):
    one, third = np.float32(1), np.float32(1.0) / np.float32(3.0)
    return (third * (a - one)) * (a - one) + (a - one) * b + b * b


def get_logo(acc, maxv, clean):
    """Normalize(maxv), GetAB per sample, GetLogo's clean-up.  acc: ScanAccumulator.  Returns the six planes aY, bY, aU, bU, aV, bV
    as one float32 array (the layout of orc_logo_create), or None where the reference throws "Insufficient logo frames"."""
    w, h = acc.w, acc.h
    wc, hc = w >> 1, h >> 1
    n = float(acc.nframes)
    m1, m2 = float(maxv), float(maxv) * maxv
    bounds = (0, w * h, w * h + wc * hc, w * h + 2 * wc * hc)
    planes = []
    with np.errstate(all="ignore"):
        for k in range(3):
            px = acc.px[bounds[k]:bounds[k + 1]].astype(np.float64)
            sF, sF2, sFB = px[:, 0] / m1, px[:, 1] / m2, px[:, 2] / m2
            sB, sB2 = float(acc.plane[2 * k]) / m1, float(acc.plane[2 * k + 1]) / m2
            A1, B1 = _approxim_line(n, sF, sB, sF2, sFB)
            A2, B2 = _approxim_line(n, sB, sF, sB2, sFB)
            A = ((A1 + (1 / A2)) / 2).astype(np.float32)
            B = ((B1 + (-B2 / A2)) / 2).astype(np.float32)
            if not (np.isfinite(A).all() and np.isfinite(B).all()) or (A == 0).any():
                return None
            planes += [A, B]
    aY, bY, aU, bU, aV, bV = planes
    if clean:
        up = lambda p: np.repeat(np.repeat(p.reshape(hc, wc), 2, axis=0), 2, axis=1).ravel()
        dist = (_calc_dist(aY, bY) + _calc_dist(up(aU), up(bU))) + _calc_dist(up(aV), up(bV))
        dist = dist * np.float32(1000)
        assert dist.dtype == np.float32
        weak = dist < np.float32(0.3)                                    # (maxfilter never changes dist: a no-op, as in the oracle)
        weakc = weak.reshape(hc, 2, wc, 2).any(axis=(1, 3)).ravel()      # a chroma sample is reset by any of its four luma pixels
        aY[weak], bY[weak] = 1, 0
        aU[weakc], bU[weakc], aV[weakc], bV[weakc] = 1, 0, 1, 0
    return np.concatenate([aY, bY, aU, bU, aV, bV]).astype(np.float32)


def _min_fades(orc, data, crops_y, w, h, bits):
    """index of the first minimum of |EvaluateLogo| over fades 0.1f * fi, fi < 20, per kept frame"""
    L = orc.lib
    lo = L.orc_logo_create(w, h, 1, 1, w, h, 0, 0, _ptr(data))
    de = L.orc_logo_deint(lo)
    L.orc_logo_create_mask(de, 0.1, 1)
    deint = L.orc_deint_y_u8 if bits <= 8 else L.orc_deint_y_u16
    mem, work = np.zeros(w * h + 8, np.float32), np.zeros(w * h + 8, np.float32)
    maxv = float((1 << bits) - 1)
    out = []
    for y in crops_y:
        deint(_ptr(mem), _ptr(y), w, w, h)
        best, idx = np.float32(np.finfo(np.float32).max), 0
        for fi in range(20):
            fade = np.float32(0.1) * np.float32(fi)
            r = np.abs(np.float32(L.orc_evaluate_logo(de, _ptr(mem), maxv, float(fade), _ptr(work), -1)))
            if r < best:
                best, idx = r, fi
        out.append(idx)
    L.orc_logo_free(de)
    L.orc_logo_free(lo)
    return out


def scanlogo(orc, clip, bits, imgw, imgh, imgx, imgy, w, h, thy, quota, path=None, serviceid=0, rect_only=False):
    """ScanLogo over numpy planes clip = {"Y", "U", "V"} of shape (n, rows, pitch).  rect_only: the planes hold the rectangle alone.
    Returns (lgd bytes or None, info); info = {"kept", "nread", "rounds": [frames re-accumulated in round 1, round 2], "data"}.
    None when the regression fails.  path: where the .lgd is written (needed for the bytes)."""
    x0, y0 = (0, 0) if rect_only else (imgx, imgy)
    maxv = (1 << bits) - 1
    acc = ScanAccumulator(w, h, thy)
    crops, nread = [], 0
    for i in range(clip["Y"].shape[0]):
        if len(crops) >= quota:
            break
        nread += 1
        Y = clip["Y"][i, y0:y0 + h, x0:x0 + w]
        U = clip["U"][i, y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2]
        V = clip["V"][i, y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2]
        if acc.add(Y, U, V):
            crops.append(tuple(np.ascontiguousarray(p) for p in (Y, U, V)))
    info = {"kept": len(crops), "nread": nread, "rounds": [], "data": None}
    data = get_logo(acc, maxv, False) if crops else None
    for _ in range(2):
        if data is None:
            return None, info
        fades = _min_fades(orc, data, [c[0] for c in crops], w, h, bits)
        acc = ScanAccumulator(w, h, thy)
        used = 0
        for c, f in zip(crops, fades):
            if f > 8:
                assert acc.add(*c)
                used += 1
        info["rounds"].append(used)
        data = get_logo(acc, maxv, True) if used else None
    if data is None:
        return None, info
    info["data"] = data
    if path is None:
        return None, info
    lo = orc.lib.orc_logo_create(w, h, 1, 1, imgw, imgh, imgx, imgy, _ptr(data))
    assert orc.lib.orc_logo_save(lo, str(path).encode(), b"No Name", serviceid) == 1
    orc.lib.orc_logo_free(lo)
    with open(path, "rb") as f:
        return f.read(), info


def write_raw_clip_hibit(path, Y, U, V, W, H, bits):
    """raw clip file of 9..12-bit frames: int32 LE {'AMTH', w, h, n, bits} + tight Y, U, V per frame as little-endian uint16"""
    n = Y.shape[0]
    with open(path, "wb") as f:
        f.write(np.array([0x48544D41, W, H, n, bits], "<i4").tobytes())
        for i in range(n):
            f.write(np.ascontiguousarray(Y[i, :, :W]).astype("<u2").tobytes())
            f.write(np.ascontiguousarray(U[i, :, :W // 2]).astype("<u2").tobytes())
            f.write(np.ascontiguousarray(V[i, :, :W // 2]).astype("<u2").tobytes())
