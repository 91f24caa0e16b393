"""The linear analysis kernel held to the reference's own rounding, so that a fault in ONE mask pixel shows.

Every other GPU check of `logo_eval_linear_kernel` / `logo_eval_linear_kernel16` allows 1e-4 or the library's own bound (2.4e-3 for the bench
logo); a score is a sum over 10^3 .. 10^4 mask pixels, so a pixel left out of a tile, a window read one column off, a wrong tap or a wrong bin
for one (pixel, fade) hides far below that.  Here every one of the 33 scores of every frame is within tol(case) = K * own(case) of the CPU
oracle's, own = the oracle's own distance from a float64 evaluation of the same terms (tests/linear_terms_ref.py: K = 8 from DESIGN section 4's
count of roundings, about 1e-5).  tests/test_linear_terms_ref_host.py shows what that buys: at this tolerance a single-pixel fault moves some
score of the case beyond reach for 95 % of the pixels (80 % for one wrong window column).

The cases are the smallest shapes that reach every staging class of the tile plan (linear_terms_ref.SHAPES), 352-wide frames:

  36 x 20 at (224, 18)              one band, three tiles, idle waves               8, 10, 16 bits
  96 x 48 at (224, 18)              three bands, the last one short                 8, 10, 16
  98 x 44 at (222, 18)              w % 4 == 2: the last staging unit moved left    8, 10
  96 x 48 at (226, 22)              origin 2 mod 4                                  8, 10
  36 x 100 at (300, 40), 288 rows   many short bands                                8, 10
  96 x 48, maskratio 1.0            every pixel, full tiles                         8, 10

each on eight noise frames (twelve above 8 bits), and the 96 x 48 logo at 8 and 10 bits (maskratio 0.30) on the edge frame set of
linear_terms_ref.case_clip, which puts a few percent of its (pixel, fade) pairs next to a bin edge: the fix-up queue's regime, at queue sizes
256 and 16.

A failure names the worst scores by frame, logo and fade and, per logo, the single-pixel mutants (term dropped, window a column to the right,
one column holding its neighbour's samples, bin one too high) that explain ALL its scores best, with what each leaves unexplained: the right
pixel leaves about 1e-6, every other about the fault's own size (FramesRef.locate).
"""
import json

import numpy as np
import pytest

import linear_terms_ref as R
from test_gpu_parity import gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def device_case(gpu, ref):
    from amatsukaze_amd import DeviceClip, Logo
    torch = gpu["torch"]
    LW, LH, X, Y0, H = ref.geom
    Y = torch.from_numpy(ref.Y.view(np.uint8 if ref.bits <= 8 else np.int16)).to(gpu["dev"])
    return DeviceClip(Y, None, None, R.W_FRAME, H, ref.bits), Logo.from_planes(gpu["ctx"], ref.data, LW, LH, R.W_FRAME, H, X, Y0)


def run_profiled(ctx, an, dclip):
    ctx.profile(True)
    try:
        got = an.analyze(dclip)
        used = sorted(k for k, (calls, _) in ctx.profile_report().items() if calls)
    finally:
        ctx.profile(False)
    return got, used


def check_guarded(ctx, ref, logo, dclip, queue=None):
    """the guarded mode: the oracle's bytes on the frames it refined, tol on the others, the exact mode's fades"""
    from amatsukaze_amd import AMTAnalyzeLogo, AMTEraseLogo
    an = AMTAnalyzeLogo(ctx, logo, ref.ratio, mode="linear")
    if queue is not None:
        an.set_fixup_queue(queue)
    got = an.analyze(dclip)
    refined = an.last_refined()
    what = "linear (guarded%s)" % ("" if queue is None else ", queue %d" % queue)
    worst = ref.check(got, what)
    as_oracle = (got.view(np.uint32) == ref.want.view(np.uint32)).all(axis=1)
    assert refined <= as_oracle.sum(), (what, refined, int(as_oracle.sum()))           # a refined frame carries the oracle's bytes
    er = AMTEraseLogo(ctx, logo, "", 0, 16)
    assert er.calc_fades(got, ref.N).tobytes() == er.calc_fades(ref.want, ref.N).tobytes(), what
    return worst, refined


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_linear_scores_within_the_references_own_rounding(gpu, case):
    from amatsukaze_amd import AMTAnalyzeLogo
    ctx = gpu["ctx"]
    ref = R.case_ref(case)
    dclip, logo = device_case(gpu, ref)
    # the exact mode's records are the oracle's bytes: the case list is honest for the kernel the linear one shares its tables with
    assert AMTAnalyzeLogo(ctx, logo, ref.ratio).analyze(dclip).tobytes() == ref.want.tobytes()
    raw = AMTAnalyzeLogo(ctx, logo, ref.ratio, mode="linear_unguarded")
    if case[2] == "edges":
        # (at 256 only: a wave whose queue runs over leaves its frames to the exact kernel, which the unguarded mode never runs -- the pairs
        #  beyond a queue of 16 would simply keep their tentative bins)
        raw.set_fixup_queue(256)
    got, used = run_profiled(ctx, raw, dclip)
    assert any(k.startswith("logo_eval_linear_kernel") for k in used) and not any("fused" in k for k in used), used
    err = np.abs(got.astype(np.float64) - ref.want.astype(np.float64))
    figures = {"case": R.case_id(case), "own": ref.own, "tol": ref.tol, "max_error": float(err.max()),
               "max_error_by_logo": [float(err[:, R.NF * k:R.NF * (k + 1)].max()) for k in range(3)], "frames": ref.N,
               "mask_pixels": [T.count for T in ref.tables]}
    print("linear_per_pixel " + json.dumps(figures))
    ref.check(got, "linear_unguarded")
    refined_at = {}
    for queue in ((256, 16) if case[2] == "edges" else (None,)):
        worst, refined = check_guarded(ctx, ref, logo, dclip, queue)
        refined_at[queue] = refined
        print("  guarded%s: max error %.3e, refined %d of %d" % ("" if queue is None else " (queue %d)" % queue, worst, refined, ref.N))
    if case[2] == "edges":
        # the queue is in use: some (logo, frame) of the set lists more than 4 x 16 pairs (tests/test_linear_terms_ref_host.py), so at 16
        # entries a wave runs over and its frame goes to the exact kernel; at 256 none does
        assert refined_at[16] > refined_at[256], refined_at
    elif ref.bits <= 10:
        # the guard is for the rare close calls, not a crutch (as tests/test_gpu_parity.py::test_analyze_linear_guarded_mode).  At 16 bits the
        # library's own bound is so wide that the guard re-evaluates every frame: only the unguarded run above says anything there.
        assert refined_at[None] <= ref.N // 4, refined_at
