"""The analysis score term by term, in numpy: the reference for the per-pixel net of the linear analysis kernel.

Checker side only, no GPU.  A score of AMTAnalyzeLogo is a sum over 10^3 .. 10^4 mask pixels divided by blackScore, so a kernel fault that is
confined to one mask pixel -- a pixel left out of a tile, a window read one column off, a wrong tap, a wrong bin for one (pixel, fade) --
moves it by far less than the 1e-4 the other linear-mode tests allow.  This module states the score twice from `Oracle.logo_arrays()`:

  score_f32    in fp32 in the reference's order ("Why the float scores are bit-exact"; oracle/amt_oracle.cpp corr_avx and
               correlation_score): blend, column sums ((r0+r1)+(r2+r3))+r4, horizontal ((c0+c4)+c2)+(c1+c3), /25, the 25 products, the same
               two sums, (int)mean clamped and >> 3, clamp(s*scale, -1, 1)*scale2, terms added front to back, / blackScore.  Byte for byte
               orc_evaluate_logo's result (tests/test_linear_terms_ref_host.py), which is what proves the statement.
  terms_f64    the same in float64 from the float64 blend, with the bins of the fp32 means (a bin edge cannot separate the two), returning
               every pixel's term.

From them: `own`, the largest |fp32 statement - float64 statement| of a case = the reference's own distance from the true value;
`tol = K * own`; and four single-pixel mutants of the float64 statement.  A mutant is killed at `tol` if it moves at least one score of the
case by more than 2 * tol: the kernel under test may sit anywhere within tol of the reference, so only a move beyond 2 * tol cannot hide.

K = 8 is not a measured number.  DESIGN section 4 charges the linear kernel 58 + 24 roundings per correlation (two window evaluations, the
interpolation, 19 + 3 on the mean) where the reference's evaluation makes about 30, and both add their terms in fp32 in some order: a factor
of about 3 over `own`; K = 8 leaves 2.7 times that.

What is fixed here and why:
  * the mutants keep the bin of the unmutated fp32 mean (except `bin+1` itself): a mutant states ONE fault;
  * `drop`, `shift` and `col` are counted over the mask pixels that are not dead (a dead pixel's scale2 is 0 in all 32 bins: its term is 0
    whatever is read); `bin+1` over the pixels that are neither dead nor at bin 31 in every (frame, fade) of the case -- min(31, bin + 1) is
    no fault there.  (The issue's rule is "term 0 for every frame, fade and bin": both rules above leave out no pixel that one does not, and
    more only where the mutant cannot be a fault.)  What is left out is counted, printed and part of every assertion's message;
  * clips of more than 8 bits get four DIM frames behind the eight: the reference clamps the mean to 255 CONTAINER units before it takes the
    bin and scales its tables for 8 bits whatever the depth, so on an ordinary 10- or 16-bit picture every bin is 31 and nearly every term
    sits on the clamp at +-scale2 -- the bin, and much of the window, cannot reach a score there.  Only a picture whose container values
    stay below 256 has bins and unclamped terms at those depths; the dim frames are the case's own 8-bit picture (logo blended at the 8-bit
    scale, +-6 of noise) in the deep container.  Without them `bin+1` is killed for 3 % of the 16-bit pixels, with them for 99 %.
"""
from __future__ import annotations

import functools

import numpy as np

from amtlib import Oracle, _decl, _ptr, c_i, c_p      # (puts tools/ on the path)
import amt_synth as S

K = 8
NF = 11
MUTANTS = ("drop", "shift", "col", "bin+1")
SHARES = {"drop": 0.95, "shift": 0.95, "col": 0.80, "bin+1": 0.95}
W_FRAME = 352
f32 = np.float32

# ---- the cases (tests/test_gpu_linear_per_pixel.py runs every one of them on the kernel) -----------------------------------------------
# name: (LW, LH, X, Y0, frame height, maskratio, depths, what it reaches)
SHAPES = {
    "w36_one_band": (36, 20, 224, 18, 240, 0.35, (8, 10, 16), "one band, three tiles, idle waves"),
    "w96_three_bands": (96, 48, 224, 18, 240, 0.35, (8, 10, 16), "three bands, the last one short"),
    "w98_ragged": (98, 44, 222, 18, 240, 0.35, (8, 10), "w % 4 == 2: the last staging unit moved left"),
    "w96_origin_mod4_2": (96, 48, 226, 22, 240, 0.35, (8, 10), "origin 2 mod 4"),
    "w36_tall": (36, 100, 300, 40, 288, 0.35, (8, 10), "many short bands"),
    "w96_every_pixel": (96, 48, 224, 18, 240, 1.0, (8, 10), "every pixel, full tiles"),
}
CASES = [(name, bits, "noise") for name, v in SHAPES.items() for bits in v[6]] + [("w96_three_bands", 8, "edges"), ("w96_three_bands", 10, "edges")]
N_NOISE = 8
EDGE_LEVELS = (16, 24, 128, 235)
EDGE_FADES = (3, 5, 7)
EDGE_RATIO = 0.30
N_DIM = 4


def case_id(case):
    return "%s-%d-%s" % case


def small_logo(w, h):
    """amt_synth.make_logo keeps an 8-pixel ring of every logo clear and draws a glyph per 40 columns: of a 36 x 20 logo (field logos 36 x 10)
    two rows would be left.  Logos narrower than 64 get a dense text-like pattern instead -- strokes of alpha up to 0.5 on a clear ground, a
    clear 2-pixel ring -- laid out as make_logo's planes (aY, bY, aU, bU, aV, bV: AMTLogo.hpp:204-212)."""
    yy, xx = np.mgrid[0:h, 0:w]
    stroke = (((xx + 2 * yy) % 9) < 3) | (((3 * xx - yy) % 14) < 2)
    alpha = np.where(stroke, 0.12 + 0.038 * ((xx * 3 + yy * 5) % 11), 0.0).astype(np.float64)
    alpha[:2, :] = 0; alpha[-2:, :] = 0; alpha[:, :2] = 0; alpha[:, -2:] = 0
    cY, cC = 235.0 / 255.0, 128.0 / 255.0
    aY = (1.0 / (1.0 - alpha)).astype(f32)
    bY = (-alpha * cY / (1.0 - alpha)).astype(f32)
    alphaUV = alpha.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    aC = (1.0 / (1.0 - alphaUV)).astype(f32)
    bC = (-alphaUV * cC / (1.0 - alphaUV)).astype(f32)
    return np.concatenate([aY.ravel(), bY.ravel(), aC.ravel(), bC.ravel(), aC.ravel(), bC.ravel()]).astype(f32), alpha, alphaUV


def case_logo(name):
    LW, LH = SHAPES[name][:2]
    return small_logo(LW, LH) if LW < 64 else S.make_logo(LW, LH)


def case_seed(case):
    name, bits, kind = case
    return 0x5EED0100 + 16 * sorted(SHAPES).index(name) + {8: 0, 10: 1, 16: 2}[bits] + (8 if kind == "edges" else 0)


def noise_frames(case, alpha, alphaUV, amp, ndim=N_DIM):
    """8 frames of make_clip_np (period 4, fade 2, flat_every 3) plus uniform noise of +-amp levels (scaled to the depth) on the luma and
    behind them, above 8 bits, ndim dim frames (module docstring)"""
    name, bits, kind = case
    LW, LH, X, Y0, H = SHAPES[name][:5]
    maxv, sh = (1 << bits) - 1, bits - 8
    Y = S.make_clip_np(N_NOISE, W_FRAME, H, case_seed(case), alpha, alphaUV, X, Y0, bits=bits, period=4, fade=2, flat_every=3)["Y"]
    rng = np.random.default_rng(case_seed(case))
    noise = rng.integers(-amp << sh, (amp << sh) + 1, size=Y.shape)
    Y = np.clip(Y.astype(np.int64) + noise, 0, maxv).astype(Y.dtype)
    if bits > 8:
        dim = S.make_clip_np(ndim, W_FRAME, H, case_seed(case), alpha, alphaUV, X, Y0, bits=8, period=4, fade=2, flat_every=3)["Y"]
        dim = np.clip(dim.astype(np.int64) + rng.integers(-amp, amp + 1, size=dim.shape), 0, 255)
        Y = np.concatenate([Y, dim.astype(Y.dtype)])
    return Y


def case_clip(case, alpha, alphaUV, data=None):
    """The luma planes of a case, (N, H, 352) u8 / u16.  "noise": noise_frames with +-6 levels.

    "edges", the regime of the kernel's fix-up queue, three groups of frames:
      * flat levels 16, 24, 128, 235 with the logo blended at alpha * 0.5;
      * for every bin edge C (8-bit: 16, 24 .. 232; deeper: 8, 16 .. 240 CONTAINER units -- the reference's bins end at 255 of those) a frame
        that is flat AT ONE FADE: s = round((C - f b maxv) / (1 - f + f a)) over the rectangle, f = 0.3, 0.5, 0.7 in turn, so that the blend
        f bg + (1 - f) s of the field logos is C up to the rounding of s and the window means at that fade -- and at no other -- scatter
        over a tenth of a level around the edge: a few percent of them within the kernel's margin, a hundred and more per (logo, frame);
      * noise_frames with +-12 levels: the frames above carry the logo's shape and nothing else, the addressing mutants need texture
        (+-6 leaves `col` at 0.71 of the pixels of the 8-bit set).
    The set runs at maskratio 0.30: at 0.35 its 10-bit tolerance, 3.8e-5 from the flat 235 frame's rounding, leaves `bin+1` at 0.949 of the pixels."""
    name, bits, kind = case
    LW, LH, X, Y0, H = SHAPES[name][:5]
    maxv = (1 << bits) - 1
    sh = bits - 8
    if kind == "noise":
        return noise_frames(case, alpha, alphaUV, 6)
    dt = np.uint8 if bits <= 8 else np.uint16
    frames = []
    U = np.zeros((H // 2, W_FRAME // 2), dt)
    for lv in EDGE_LEVELS:
        Y = np.full((H, W_FRAME), lv << sh, dt)
        S.blend_logo_np(Y, U, U.copy(), alpha, alphaUV, X, Y0, 0.5, bits)
        frames.append(Y)
    a = data[:LW * LH].reshape(LH, LW).astype(np.float64)
    b = data[LW * LH:2 * LW * LH].reshape(LH, LW).astype(np.float64)
    for i, C in enumerate(range(16, 240, 8) if bits <= 8 else range(8, 248, 8)):
        f = EDGE_FADES[i % len(EDGE_FADES)] / 10.0
        Y = np.full((H, W_FRAME), C, np.float64)
        Y[Y0:Y0 + LH, X:X + LW] = np.rint((C - f * b * maxv) / (1 - f + f * a))
        frames.append(np.clip(Y, 0, maxv).astype(dt))
    return np.concatenate([np.stack(frames), noise_frames(case, alpha, alphaUV, 12)])


# ---- tables --------------------------------------------------------------------------------------------------------------------------
class LogoTables:
    """One evaluation logo (deint, top field or bottom field) as orc_logo_create_mask left it."""

    def __init__(self, orc, handle):
        o = orc.logo_info(handle)
        self.w, self.h = int(o[0]), int(o[1])
        data, mask, ker, sc, black, mp, cnt = orc.logo_arrays(handle)
        w, h = self.w, self.h
        self.a = data[:w * h].reshape(h, w).copy()
        self.b = data[w * h:2 * w * h].reshape(h, w).copy()
        self.black = f32(black)
        m = mask.reshape(h, w).astype(bool).copy()
        m[:2] = False; m[-2:] = False; m[:, :2] = False; m[:, -2:] = False          # correlation_score walks the interior only
        self.ys, self.xs = np.nonzero(m)                                             # raster order = the tables' order
        self.count = cnt
        assert len(self.xs) == cnt, (len(self.xs), cnt)
        self.taps = ker[:cnt * 25].reshape(cnt, 5, 5).copy()                          # [dy + 2][dx + 2]
        sc = sc[:cnt * 64].reshape(cnt, 32, 2)
        self.scale, self.scale2 = sc[:, :, 0].copy(), sc[:, :, 1].copy()
        self.dead = ~((self.scale * self.scale2) != 0).any(axis=1)
        d = np.arange(-2, 3)
        self.rows = (self.ys[:, None, None] + d[None, :, None]) + np.zeros((1, 1, 5), np.int64)
        self.cols = (self.xs[:, None, None] + d[None, None, :]) + np.zeros((1, 5, 1), np.int64)


def _sum5(r, axis):
    """((r0+r1)+(r2+r3))+r4 along `axis` -- corr_avx's column sums"""
    t = np.moveaxis(r, axis, 0)
    return ((t[0] + t[1]) + (t[2] + t[3])) + t[4]


def _hsum(c):
    """((c0+c4)+c2)+(c1+c3) over the last axis -- hsum8 with lanes 5..7 zero"""
    return ((c[..., 0] + c[..., 4]) + c[..., 2]) + (c[..., 1] + c[..., 3])


def blend(T, src, maxv, fade, dt):
    """EvaluateLogo's work plane (LogoScan.hpp:231-255) in `dt`; fade is the reference's fp32 value in both"""
    src = src.astype(dt)
    fade = dt(f32(fade))
    bg = T.a.astype(dt) * src + T.b.astype(dt) * dt(maxv)
    return fade * bg + (dt(1) - fade) * src


def window_stats(T, win, dt):
    """(mean, correlation) of the windows `win` (count, 5, 5) in `dt`, in the reference's order"""
    mean = _hsum(_sum5(win, 1)) / dt(25)
    prod = T.taps.astype(dt) * (win - mean[:, None, None])
    return mean, _hsum(_sum5(prod, 1))


def bins_of(mean):
    """(int)mean clamped to [0, 255] >> 3 for finite means (LogoScan.hpp:304)"""
    return np.clip(np.trunc(mean.astype(np.float64)), 0, 255).astype(np.int64) >> 3


def terms_of(T, corr, bins, dt):
    n = np.arange(len(bins))
    s = corr * T.scale[n, bins].astype(dt)
    return np.maximum(dt(-1), np.minimum(dt(1), s)) * T.scale2[n, bins].astype(dt)


def score_f32(T, src, maxv, fade):
    """orc_evaluate_logo(T, src, maxv, fade) in numpy fp32: (score, fp32 means, bins)"""
    work = blend(T, src, maxv, fade, f32)
    mean, corr = window_stats(T, work[T.rows, T.cols], f32)
    bins = bins_of(mean)
    terms = terms_of(T, corr, bins, f32)
    total = np.cumsum(terms, dtype=f32)[-1] if len(terms) else f32(0)            # front to back, fp32
    return f32(total) / T.black, mean, bins


def terms_f64(T, src, maxv, fade, bins, mutant=None):
    """Every mask pixel's term in float64 from the float64 blend with the given bins.  `mutant`: the same with the named fault applied to
    EVERY pixel at once -- element p of the result is what pixel p's term becomes when p alone is faulty."""
    f64 = np.float64
    work = blend(T, src, maxv, fade, f64)
    if mutant == "drop":
        return np.zeros(T.count, f64)
    cols = np.minimum(T.cols + 1, T.w - 1) if mutant == "shift" else T.cols
    win = work[T.rows, cols]
    if mutant == "col":
        win = win.copy()
        win[:, :, 4] = win[:, :, 3]
    if mutant == "bin+1":
        bins = np.minimum(31, bins + 1)
    _, corr = window_stats(T, win, f64)
    return terms_of(T, corr, bins, f64)


# ---- a case: frames, the oracle's records, own, tol, the mutants' moves ---------------------------------------------------------------------
class FramesRef:
    """The oracle's records of luma planes Y (N, H, pitch) under a logo, the two statements, `own`, `tol` and (mutants=True) what every
    single-pixel mutant does to every score.  `label` names the frames in messages."""

    def __init__(self, label, data, geom, ratio, bits, Y, W=W_FRAME, mutants=True):
        self.label, self.data, self.Y, self.with_mutants = label, data, Y, mutants
        LW, LH, X, Y0, H = geom
        self.bits, self.ratio, self.geom = bits, ratio, geom
        self.maxv = float((1 << bits) - 1)
        N = self.N = self.Y.shape[0]
        orc = self.orc = Oracle()
        L = orc.lib
        _decl(L, "orc_copy_y_u16", None, [c_p, c_p, c_i, c_i, c_i])
        lo = orc.make_logo(self.data, LW, LH, W, H, X, Y0)
        d = L.orc_logo_deint(lo); L.orc_logo_create_mask(d, ratio, 1)
        t = L.orc_logo_field(lo, 0); L.orc_logo_create_mask(t, ratio, 1)
        b = L.orc_logo_field(lo, 1); L.orc_logo_create_mask(b, ratio, 1)
        self.handles = (d, t, b)
        self.tables = tuple(LogoTables(orc, h) for h in self.handles)
        want = np.zeros(N * 33, f32)
        L.orc_analyze_frames(d, t, b, _ptr(self.Y), self.Y.strides[0], self.Y.shape[2], bits, N, _ptr(want))
        self.want = want.reshape(N, 33)
        # the source planes as orc_analyze_frames forms them (LogoScan.hpp:1100-1161): DeintY for the deint logo, CopyY's even / odd rows
        copy, deint = (L.orc_copy_y_u8, L.orc_deint_y_u8) if bits <= 8 else (L.orc_copy_y_u16, L.orc_deint_y_u16)
        self.src = []
        for n in range(N):
            rect = np.ascontiguousarray(self.Y[n, Y0:Y0 + LH, X:X + LW])
            mc, md = np.zeros((LH, LW), f32), np.zeros((LH, LW), f32)
            copy(_ptr(mc), _ptr(rect), LW, LW, LH)
            deint(_ptr(md), _ptr(rect), LW, LW, LH)
            self.src.append((md, mc[0::2].copy(), mc[1::2].copy()))
        self.fades = [f32(f) / f32(10) for f in range(NF)]
        self._evaluate()

    def _evaluate(self):
        N = self.N
        self.s32 = np.zeros((N, 3, NF), f32)                     # signed fp32 statement
        self.s64 = np.zeros((N, 3, NF))                           # signed float64 statement
        self.mean32 = [np.zeros((N, NF, T.count), f32) for T in self.tables]
        self.bins = [np.zeros((N, NF, T.count), np.int64) for T in self.tables]
        # delta[k][m][n, f, p]: what mutant m of pixel p of logo k adds to the SIGNED score (n, k, f)
        self.delta = [{m: np.zeros((N, NF, T.count)) for m in (MUTANTS if self.with_mutants else ())} for T in self.tables]
        for k, T in enumerate(self.tables):
            black = float(T.black)
            for n in range(N):
                for f, fade in enumerate(self.fades):
                    sc, mean, bins = score_f32(T, self.src[n][k], self.maxv, fade)
                    self.s32[n, k, f] = sc
                    self.mean32[k][n, f], self.bins[k][n, f] = mean, bins
                    t = terms_f64(T, self.src[n][k], self.maxv, fade, bins)
                    self.s64[n, k, f] = t.sum() / black
                    for m in self.delta[k]:
                        self.delta[k][m][n, f] = (terms_f64(T, self.src[n][k], self.maxv, fade, bins, m) - t) / black
        self.own = float(np.abs(np.abs(self.s32.astype(np.float64)) - np.abs(self.s64)).max())
        self.tol = K * self.own

    def records_f32(self):
        """the fp32 statement laid out as orc_analyze_frames' records"""
        return np.abs(self.s32).reshape(self.N, 33)

    def moves(self, k, m):
        """largest move of any |score| of the case under mutant m of each pixel of logo k: (count,)"""
        s = self.s64[:, k, :, None]
        return np.abs(np.abs(s + self.delta[k][m]) - np.abs(s)).max(axis=(0, 1))

    def population(self, k, m):
        T = self.tables[k]
        if m == "bin+1":
            return ~T.dead & (self.bins[k] < 31).any(axis=(0, 1))
        return ~T.dead

    def kill_shares(self, tol):
        """{mutant: (killed, counted, left out)} pooled over the three logos"""
        out = {}
        for m in MUTANTS:
            killed = counted = 0
            for k, T in enumerate(self.tables):
                pop = self.population(k, m)
                killed += int((self.moves(k, m)[pop] > 2 * tol).sum())
                counted += int(pop.sum())
            out[m] = (killed, counted, sum(T.count for T in self.tables) - counted)
        return out

    def near_edge(self, margin_levels=1e-3):
        """Means at the fades 1..9 within margin_levels * maxv / 255 of a multiple of 8 that separates two bins (8 .. 248), over the three
        logos: (share of the (pixel, fade) pairs that are there in some frame, share of the (pixel, frame, fade) triples, most fades of one
        (pixel, frame), most triples of one (logo, frame)).  The kernel's own margin is 22 u v, v = max(1, |a| + |b|) * maxv: 1.3e-3 *
        maxv / 255 for the suite's logo ("Bins")."""
        hits = pairs = triples = hit_pairs = most = crowd = 0
        for k in range(3):
            mean = self.mean32[k][:, 1:10].astype(np.float64)
            edge = np.clip(np.rint(mean / 8.0), 1, 31) * 8.0
            near = np.abs(mean - edge) <= margin_levels * self.maxv / 255.0
            hits += int(near.sum()); triples += near.size
            hit_pairs += int(near.any(axis=0).sum()); pairs += near[0].size
            most = max(most, int(near.sum(axis=1).max()))
            crowd = max(crowd, int(near.sum(axis=(1, 2)).max()))
        return hit_pairs / pairs, hits / triples, most, crowd

    def locate(self, k, diff, limit=3):
        """The single-pixel mutants of logo k that explain `diff` (N, 11) = got - oracle over ALL scores of the group at once, best first:
        [(largest |mutant's move - diff| over the group's scores, mutant, x, y)].  A fault in one pixel moves every score of its logo the
        way ONE mutant of ONE pixel does, so the right candidate leaves a residual near tol while every other leaves about |diff|."""
        T = self.tables[k]
        s = self.s64[:, k, :, None]
        cand = []
        for m, delta in self.delta[k].items():
            resid = np.abs((np.abs(s + delta) - np.abs(s)) - diff[:, :, None]).max(axis=(0, 1))
            cand += [(float(resid[p]), m, int(T.xs[p]), int(T.ys[p])) for p in np.argsort(resid)[:limit]]
        return sorted(cand)[:limit]

    def check(self, got, what):
        """every score of `got` (N, 33) within tol of the oracle's, or an AssertionError that names the worst scores by frame, logo and fade
        and, per logo, the single-pixel mutants that would explain the differences"""
        names = ("deint", "top field", "bottom field")
        diff = got.astype(np.float64) - self.want.astype(np.float64)
        err = np.abs(diff)
        bad = np.argwhere(~(err <= self.tol))
        if len(bad) == 0:
            return float(err.max())
        lines = []
        for n, j in bad[np.argsort(-err[tuple(bad.T)])][:4]:
            k, f = divmod(int(j), NF)
            lines.append("frame %d, %s logo, fade %d: %.9g against the oracle's %.9g (%+.3e)" % (n, names[k], f, got[n, j], self.want[n, j], diff[n, j]))
        for k in sorted({int(j) // NF for _, j in bad}):
            d = diff[:, NF * k:NF * (k + 1)]
            found = self.locate(k, d) if np.isfinite(d).all() else []
            lines.append("%s logo, largest difference %.3e; single-pixel mutants that explain all its scores best: %s" % (names[k], float(np.abs(d).max()), "; ".join(
                "%s at (x %d, y %d) leaves %.2e" % (m, x, y, r) for r, m, x, y in found) or "none evaluated"))
        raise AssertionError("%s, %s: %d of %d scores beyond tol = %d * own = %.3e (max error %.3e)\n  " % (what, self.label, len(bad), err.size, K, self.tol, float(np.nanmax(err)))
                             + "\n  ".join(lines))


class CaseRef(FramesRef):
    """Everything about a case that needs no GPU; built once per process and shared (case_ref)."""

    def __init__(self, case):
        self.case = case
        name, bits, kind = case
        self.data, self.alpha, self.alphaUV = case_logo(name)
        FramesRef.__init__(self, "case " + case_id(case), self.data, SHAPES[name][:5], EDGE_RATIO if kind == "edges" else SHAPES[name][5], bits, case_clip(case, self.alpha, self.alphaUV, self.data))


@functools.lru_cache(maxsize=None)
def case_ref(case):
    return CaseRef(case)
