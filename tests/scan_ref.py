"""numpy statement of LogoScan::AddFrame (LogoScan.hpp:594-660), its med_average (:414-428) and AddScanFrame (:568-592), for the tests.

Written from the reference's text in int64; tests/test_scan_ref_host.py pins it against the C++ oracle at 8 bits.  The reference is a
template over pixel_t, so for 16-bit containers the same statement holds with a wider sample: the border samples are kept in `short`,
so a 16-bit container value above 32767 enters the decision and the trimmed mean as its
two's-complement wrap (AddScanFrame still sums the real value)."""
import numpy as np


def border_samples(plane, w, h):
    """sorted border samples of the w x h rectangle at plane[0, 0]: the top and bottom rows interleaved, then the left and right columns
    of rows 1 .. h-2.  A one-row plane contributes its row twice (row 0 is also row h-1)."""
    p = np.asarray(plane)[:h, :w]
    if p.dtype == np.uint16:
        p = p.astype(np.int16)                           # tmpY.push_back(srcY[x]) into a std::vector<short>
    p = p.astype(np.int64)
    rows = np.stack([p[0], p[h - 1]], axis=1).ravel()
    cols = np.stack([p[1:h - 1, 0], p[1:h - 1, w - 1]], axis=1).ravel()
    s = np.concatenate([rows, cols])
    return np.sort(s)


def med_average(s):
    """(int)((sum of the middle half + nn/2) / nn) with the division in double"""
    n = len(s)
    mid = s[n // 4: n - n // 4]
    nn = len(mid)
    return int((float(int(mid.sum())) + nn // 2) / nn)


def add_frame(Y, U, V, w, h, thy):
    """Y, U, V: planes whose [0, 0] is the rectangle's corner.  None when a plane's border spread exceeds thy, else (bgY, bgU, bgV)."""
    bg = []
    for p, pw, ph in ((Y, w, h), (U, w >> 1, h >> 1), (V, w >> 1, h >> 1)):
        s = border_samples(p, pw, ph)
        if abs(int(s[0]) - int(s[-1])) > thy:
            return None
        bg.append(s)
    return tuple(med_average(s) for s in bg)


class ScanAccumulator:
    """sumF, sumF2, sumFB per pixel (luma rows, then U rows, then V rows) and {sumB, sumB2} per plane: the layout of LogoScan.sums()"""

    def __init__(self, w, h, thy):
        self.w, self.h, self.thy = w, h, thy
        self.npx = w * h + 2 * (w >> 1) * (h >> 1)
        self.px = np.zeros((self.npx, 3), np.int64)
        self.plane = np.zeros(6, np.int64)
        self.nframes = 0

    def add(self, Y, U, V):
        """one frame (planes starting at the rectangle's corner); True when it was accepted"""
        bg = add_frame(Y, U, V, self.w, self.h, self.thy)
        if bg is None:
            return False
        w, h = self.w, self.h
        o = 0
        for k, (p, pw, ph) in enumerate(((Y, w, h), (U, w >> 1, h >> 1), (V, w >> 1, h >> 1))):
            f = np.asarray(p)[:ph, :pw].astype(np.int64).ravel()
            self.px[o:o + f.size, 0] += f
            self.px[o:o + f.size, 1] += f * f
            self.px[o:o + f.size, 2] += f * bg[k]
            self.plane[2 * k] += bg[k]
            self.plane[2 * k + 1] += bg[k] * bg[k]
            o += f.size
        self.nframes += 1
        return True

    def sums(self):
        return self.px.ravel().copy(), self.plane.copy()
