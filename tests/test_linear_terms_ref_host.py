"""The per-pixel net of the linear analysis kernel, checker side (no GPU): tests/linear_terms_ref.py states the score term by term, and
tests/test_gpu_linear_per_pixel.py holds the kernel to tol(case) = K * own(case) of the oracle on the cases below.  Here:

  * the fp32 statement IS the oracle: its records equal orc_analyze_frames' byte for byte on every case (orc_evaluate_logo underneath);
  * the cases are a net: at tol(case) a fault in ONE mask pixel -- its term dropped, its window read a column to the right, one window column
    holding its neighbour's samples, its bin one too high -- moves some score of the case by more than 2 * tol for at least 0.95 / 0.95 /
    0.80 / 0.95 of the pixels that are not dead.  These shares are conditions on the inputs: a case that misses one gets other frames or a
    smaller mask, the threshold does not move.  The same shares at the 1e-4 of the older linear-mode tests are printed beside them;
  * the edge frame set puts a few percent of the (pixel, fade) pairs next to a bin edge in some frame: the regime of the kernel's fix-up
    queue -- and is held to the same shares.

Logos of the benchmark's size (256 x 128, 10 926 mask pixels) cannot meet these shares at any tolerance the reference supports: a pixel's
term is a ten-thousandth of the score and the reference's own fp32 rounding is 1.8e-6 there.  Measured with this module on the 256 x 128
make_logo in eight noise frames of 720 x 480: at 8 * own `drop` is killed for 0.92 of the pixels, `shift` for 0.74, `col` for 0.34 and
`bin+1` for 0.09 (at 1e-4: 0.46, 0.05, 0.04, 0).  That is why the net is made of small logos.
"""
import numpy as np
import pytest

import linear_terms_ref as R

EDGE_CASES = [c for c in R.CASES if c[2] == "edges"]


def _show(ref, tol):
    return "  ".join("%s %.3f (%d / %d, %d left out)" % (m, k / max(n, 1), k, n, out) for m, (k, n, out) in ref.kill_shares(tol).items())


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_fp32_statement_is_the_oracle(case):
    ref = R.case_ref(case)
    assert np.isfinite(ref.want).all()
    assert ref.records_f32().tobytes() == ref.want.tobytes()
    # the float64 statement is the same sum: within the reference's own rounding of it, which is far below the older tests' 1e-4
    assert 0 < ref.own < 1e-5, ref.own
    assert all(T.count > 0 for T in ref.tables)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_single_pixel_faults_are_visible_at_tol(case):
    ref = R.case_ref(case)
    shares = ref.kill_shares(ref.tol)
    print("%s: own %.3e, tol = %d * own = %.3e, mask pixels %s, dead %s" % (R.case_id(case), ref.own, R.K, ref.tol, [T.count for T in ref.tables],
                                                                          [int(T.dead.sum()) for T in ref.tables]))
    print("  killed at tol :", _show(ref, ref.tol))
    print("  killed at 1e-4:", _show(ref, 1e-4), " (before)")
    for m, (killed, counted, left_out) in shares.items():
        assert counted > 0, (m, "left out", left_out)
        assert killed >= R.SHARES[m] * counted, (m, "killed", killed, "of", counted, "left out", left_out)


@pytest.mark.parametrize("case", EDGE_CASES, ids=R.case_id)
def test_edge_frames_put_means_next_to_bin_edges(case):
    """Between 1 % and 20 % of the (pixel, fade) pairs, fades 1 .. 9, have in some frame of the set an fp32 mean within 1e-3 gray levels *
    maxv / 255 of a bin edge, and no (pixel, frame) at every fade (tests/test_gpu_eval_shapes.py::test_linear_mode_flat_frames_on_bin_edges is
    the case where all are at once).  Some (logo, frame) holds more than 4 * 16 such triples: a workgroup of the kernel is four waves on
    one logo, each with a queue of its own, so at a queue of 16 entries one of them runs over there and the frame goes to the exact kernel
    -- what tests/test_gpu_linear_per_pixel.py sees as frames refined at 16 that are not at 256."""
    ref = R.case_ref(case)
    pairs, triples, most, crowd = ref.near_edge()
    print("%s: next to an edge in some frame: %.4f of the (pixel, fade) pairs; %.2e of the triples, at most %d fades of a (pixel, frame), at most %d "
          "triples of a (logo, frame)" % (R.case_id(case), pairs, triples, most, crowd))
    assert 0.01 <= pairs <= 0.20, pairs
    assert 1 <= most < 9, most
    assert crowd > 4 * 16, crowd


def test_a_failure_names_the_pixel():
    """Records that carry one planted single-pixel fault fail the check the GPU test makes, and the message names frame, logo, fade and the
    pixel; the oracle's own records and the fp32 statement pass it."""
    ref = R.case_ref(("w96_three_bands", 8, "noise"))
    assert ref.check(ref.want, "oracle") == 0.0
    k, m = 1, "shift"
    p = int(np.argmax(ref.moves(k, m)))
    T = ref.tables[k]
    got = ref.want.copy()
    got[:, R.NF * k:R.NF * (k + 1)] = np.abs(ref.s64[:, k] + ref.delta[k][m][:, :, p]).astype(np.float32)
    with pytest.raises(AssertionError) as e:
        ref.check(got, "planted")
    msg = str(e.value)
    print(msg)
    assert "top field logo, largest difference" in msg and "best: %s at (x %d, y %d) leaves" % (m, T.xs[p], T.ys[p]) in msg
    assert ref.locate(k, (got.astype(np.float64) - ref.want)[:, R.NF * k:R.NF * (k + 1)])[0][0] < ref.tol       # ... and explains them within tol
    # with that group put back the records pass again
    got[:, R.NF * k:R.NF * (k + 1)] = ref.want[:, R.NF * k:R.NF * (k + 1)]
    assert ref.check(got, "restored") == 0.0
