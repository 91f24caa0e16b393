"""The inputs of tests/test_gpu_plane_edges.py, judged without a GPU: every input tells the true frame metrics (logo finder sums)
from each deliberately wrong kernel that applies to it (tests/plane_edge_clips.py), the two oracles of the frame metrics agree on the
new geometries, the saturated clip's records are the closed forms, and the full-range clips hold the value combinations they are
there for.  An input that cannot tell a mutant apart is not a test of it: fix the input, not the list."""
import numpy as np
import pytest

import plane_edge_clips as P
from amtlib import Oracle


@pytest.fixture(scope="module")
def orc():
    return Oracle()


_clips = {}


def clip_of(family, case):
    key = (family, P.case_id(case))
    if key not in _clips:
        _clips[key] = P.fs_clip(case, family)
    return _clips[key]


def runs_of(family, case):
    """the (batch, previous frame) pairs the GPU test runs on this case"""
    clip, sep = clip_of(family, case)
    batch = clip.sub(1)
    return [(batch, None), (batch, sep if sep is not None else clip.sub(0, 1))]


def test_parameter_lists_reach_every_form():
    assert P.forms_reached("frame_stats", P.GEOMETRY_CASES) == P.FRAME_STATS_FORMS
    # the unaligned rows go through the buffer loads, whole rows and ragged, at both sample sizes
    unaligned = {(P.predicted_form("frame_stats", W, p, es), es) for es, lst in ((1, P.UNALIGNED_8), (2, P.UNALIGNED_16)) for W, p in lst}
    assert unaligned == {(f, es) for f in ("buf", "buf_ragged") for es in (1, 2)}
    assert all((p * es) % 16 for es, lst in ((1, P.UNALIGNED_8), (2, P.UNALIGNED_16)) for W, p in lst)
    assert P.forms_reached("frame_stats", P.ADDRESSING_CASES) == P.FRAME_STATS_FORMS
    # the partial dword of the ragged 8-bit widths holds 1, 3 and 2 bytes
    assert sorted(W % 4 for W, p in P.FS_WIDTHS[8] if P.predicted_form("frame_stats", W, p, 1) == "buf_ragged") == [1, 2, 3]
    # the finder: both forms at both sample sizes; the buffer-load cases have rows (or a base) that are no multiple of the load
    assert P.forms_reached("logofind", P.LOGOFIND_CASES) == P.LOGOFIND_FORMS
    for bits, w, h, pitch, n, kw in P.LOGOFIND_CASES:
        es = 1 if bits <= 8 else 2
        assert (pitch * es) % (4 * es) or (kw.get("base", 0) * es) % (4 * es)


def test_dealing_cases_are_what_they_claim():
    """1, 3, 129 and 127 lane columns per row; workgroups of 128 threads rounded up to a multiple of 8, most of them idle in two"""
    cols = [-(-W // 16) for b, W, p, H, N, kw in P.DEALING_CASES]
    assert cols == [1, 3, 129, 127]
    for (b, W, p, H, N, kw), c in zip(P.DEALING_CASES, cols):
        assert P.predicted_form("frame_stats", W, p, 1) == "buf" and H % 24 != 0
        tiles = -(-H // 24)
        assert (tiles * c) % 128 != 0              # the last busy workgroup is partly idle
        assert 128 % c != 0 or c == 1              # waves straddle tiles (one column: 64 tiles to a wave)
    wgs = [-(-(-(-H // 24) * c) // 128) for (b, W, p, H, N, kw), c in zip(P.DEALING_CASES, cols)]
    assert any(w % 8 == 1 for w in wgs) and any(w % 8 not in (0, 1) for w in wgs), wgs      # 7 idle workgroups; some idle


@pytest.mark.parametrize("family", list(P.FS_FAMILIES))
def test_frame_metric_inputs_tell_every_mutant_apart(family):
    applied = {m: 0 for m in P.FS_FAMILY_MUTANTS[family]}
    for case in P.FS_FAMILIES[family]:
        for batch, prev in runs_of(family, case):
            want = P.true_metrics(batch, prev)
            # the model itself: without a mutation it is the specification
            assert np.array_equal(P.fs_model(batch, prev), want), (P.case_id(case), prev is not None)
            for m in applied:
                if not P.fs_mutant_applies(m, batch, prev):
                    continue
                applied[m] += 1
                got = P.fs_model(batch, prev, P.FS_MUTANTS[m])
                assert not np.array_equal(got, want), (family, P.case_id(case), m, prev is not None)
    assert all(applied.values()), applied


def test_logofind_inputs_tell_every_mutant_apart():
    applied = {m: 0 for m in P.LOGOFIND_MUTANTS}
    for case in P.LOGOFIND_CASES:
        clip = P.lf_clip(case)
        want = P.true_sums(clip)
        assert np.array_equal(P.lf_model(clip), want), P.lf_case_id(case)
        for m in applied:
            if not P.lf_mutant_applies(m, clip):
                continue
            applied[m] += 1
            assert not np.array_equal(P.lf_model(clip, P.LF_MUTANTS[m]), want), (P.lf_case_id(case), m)
    assert all(applied.values()), applied


@pytest.mark.parametrize("family", list(P.FS_FAMILIES))
def test_c_and_numpy_oracles_agree_on_the_new_geometries(orc, family):
    """odd heights, H = 4 and 5, gapped strides, offset bases, a previous frame elsewhere, 16-bit full-range containers"""
    for case in P.FS_FAMILIES[family]:
        for batch, prev in runs_of(family, case):
            assert np.array_equal(P.orc_metrics(orc, batch, case[0], prev), P.true_metrics(batch, prev)), (P.case_id(case), prev is not None)


def closed_form_records(top, W, H, N, with_prev):
    """the saturated clip (frame n: rows of parity n % 2 at `top`, the others 0), written out by hand"""
    up, dn = -(-H // 2), H // 2            # even rows, odd rows
    rec = np.zeros((N, 8), np.uint64)
    for n in range(N):
        comb = top * W * (H - 2)
        if n >= 1 or with_prev:
            # every sample differs from the previous frame's by top; inside one field nothing changes; every inner row stands
            # against two neighbours of the other value; both weaves are flat
            rec[n] = [top * W * up, top * W * dn, 0, comb, 0, 0, 0, 0]
        else:
            rec[n] = [0, 0, 0, comb, comb, 0, 0, 0]      # frame 0 against itself: the weave is the frame
        rec[n, 5] = top * W * (up if n % 2 == 0 else dn)
    return rec


@pytest.mark.parametrize("case", P.SATURATED_CASES, ids=P.case_id)
def test_saturated_clip_meets_the_closed_forms(case):
    bits, W, pitch, H, N, kw = case
    for batch, prev in runs_of("saturated", case):
        assert np.array_equal(P.true_metrics(batch, prev), closed_form_records(batch.top, W, H, N, prev is not None))


def test_largest_wave_partial_fits_32_bits():
    """a wave sums 64 lanes x 16 rows x 8 samples (24 x 16 at 8 bits) of at most the top value into 32 bits before its atomic"""
    assert 64 * 16 * 8 * 65535 < 2 ** 32 and 64 * 24 * 16 * 255 < 2 ** 32


def test_full_range_8bit_clip_holds_every_vertical_pair():
    clip, _ = clip_of("full_range_8", P.FULL_RANGE_8_CASES[0])
    assert P.vertical_pairs_8bit(clip.sub(1).frames()).all()


@pytest.mark.parametrize("case", P.FULL_RANGE_16_CASES, ids=P.case_id)
def test_full_range_16bit_clip_holds_every_edge_triple(case):
    clip, _ = clip_of("full_range_16", case)
    Y = clip.sub(1).frames()
    assert int(Y.max()) > 0x8000 and int(Y.min()) < 0x0400          # full-range containers whatever depth is declared
    r, c = P.EDGE_AT
    blk = Y[:P.EDGE_BLOCK[0], r:r + P.EDGE_BLOCK[1], c:c + P.EDGE_BLOCK[2]]
    assert c % 2 == 0 and np.array_equal(blk, P.edge_block())
    for parity in (0, 1):
        assert P.edge_triples(blk, parity) == P.all_edge_triples()
