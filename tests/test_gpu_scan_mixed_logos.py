"""LogoFrame scans over lists whose logos differ in size and position (tests/logo_sets.py), the way the `.lgd` files of different
channels do in real use.  With one shared rectangle, per-logo state of the scan path cannot be told apart: the band count, tile tables and
`out_off` a workgroup of logo_eval_pair_kernel takes for its logo, the (logo, frame group) map of one launch over logos with different
band counts, the all-or-nothing choice of the generic kernel with its single LDS plane size for whole-row and column bands, the
record stride when a slot in the middle of the list is skipped.

Every comparison is byte equality with orc_logoframe_scan over the same list (a null handle for a slot that is skipped); which kernel
ran is read from the context's profile, as test_gpu_parity.test_logoframe_scan_kernel_choice does."""
import ctypes as C

import numpy as np
import pytest

import logo_sets as LS
from amtlib import Oracle
from test_gpu_parity import SMALL, gpu, make_case  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

PAIR, GENERIC = "logo_eval_pair_kernel.scan", "logo_eval_fused_kernel.scan"
HOLE = 2                                                # the slot of the file that cannot be read in [A, B, missing, C, D, E]
WIDE = dict(W=LS.WIDE_FRAME[0], H=LS.WIDE_FRAME[1], LW=LS.WIDE_MIXED[0][0], LH=LS.WIDE_MIXED[0][1], IMGX=LS.WIDE_MIXED[0][2],
            IMGY=LS.WIDE_MIXED[0][3], N=6, period=4, fade=2, flat=3)


def with_hole(items, hole):
    return list(items[:HOLE]) + [hole] + list(items[HOLE:])


def profiled_scan(ctx, lf, scan):
    """runs scan() and returns the names of the kernels the context launched meanwhile"""
    ctx.profile(True)
    scan()
    got = lf.evalResults
    used = [k for k, (calls, _) in ctx.profile_report().items() if calls]
    ctx.profile(False)
    return got, used


class SmallMixed:
    """SMALL_MIXED in every form, the clips of test_gpu_parity.SMALL per (bits, pitch_pad) and the scan of case 1 -- each computed once"""

    def __init__(self, gpu, tmp):
        assert (SMALL["W"], SMALL["H"]) == LS.SMALL_FRAME and (SMALL["LW"], SMALL["LH"], SMALL["IMGX"], SMALL["IMGY"]) == LS.LOGO_A
        self.gpu, self.ctx, self.tmp, self.orc = gpu, gpu["ctx"], tmp, Oracle()
        self.built = LS.build(LS.SMALL_MIXED, LS.SMALL_FRAME, orc=self.orc, ctx=self.ctx, lgd_dir=tmp)
        self.missing = str(tmp / "missing.lgd")
        self._cases, self._want, self._hole_scans = {}, {}, {}

    def case(self, bits=8, pad=0):
        if (bits, pad) not in self._cases:
            self._cases[bits, pad] = make_case(self.gpu, SMALL, bits=bits, pitch_pad=pad)
        return self._cases[bits, pad]

    def want(self, bits=8, pad=0):
        """the oracle's records of [A, B, C, D, E] on the clip: [frames][5][2]"""
        if (bits, pad) not in self._want:
            self._want[bits, pad] = LS.oracle_scan(self.orc, self.built.evals, self.case(bits, pad)["clip"]["Y"], bits, LS.SMALL_FRAME)
            self._want[bits, pad].setflags(write=False)
        return self._want[bits, pad]

    def hole_scan(self, bits=8, pad=0):
        """case 1: [A, B, missing.lgd, C, D, E] as paths, scanFrames in batches of 17 -> (LogoFrame, records, kernels used)"""
        if (bits, pad) not in self._hole_scans:
            from amatsukaze_amd import LogoFrame
            lf = LogoFrame(self.ctx, with_hole(self.built.paths, self.missing), LS.MASKRATIO)
            got, used = profiled_scan(self.ctx, lf, lambda: lf.scanFrames(self.case(bits, pad)["dclip"], batch=17))
            got.setflags(write=False)
            self._hole_scans[bits, pad] = (lf, got, used)
        return self._hole_scans[bits, pad]


@pytest.fixture(scope="module")
def small(gpu, tmp_path_factory):
    return SmallMixed(gpu, tmp_path_factory.mktemp("mixed"))


# ---- 1 ----
@pytest.mark.parametrize("bits,pad", [(8, 0), (8, 32), (10, 0)])
def test_pair_kernel_mixed_list_with_a_hole(small, tmp_path, bits, pad):
    """Five logos of different geometry around a file that cannot be read, 40 frames in batches of 17 (17 + 17 + 6): one launch holds
    workgroups of every logo, each with its own band count, tiles, tables and `out_off`; the engine sees five logos while the records
    are six wide."""
    orc = small.orc
    lf, got, used = small.hole_scan(bits, pad)
    assert used == [PAIR], used
    Y = small.case(bits, pad)["clip"]["Y"]
    want = LS.oracle_scan(orc, with_hole(small.built.evals, None), Y, bits, LS.SMALL_FRAME)
    assert want[:, [0, 1, 3, 4, 5]].tobytes() == small.want(bits, pad).tobytes()         # (the oracle's own columns do not depend on the list)
    assert got.shape == want.shape == (Y.shape[0], 6, 2)
    for i in range(6):
        assert got[:, i].tobytes() == want[:, i].tobytes(), ("logo slot", i)
    assert got.tobytes() == want.tobytes()
    assert np.all(got[:, HOLE, 0] == 0) and np.all(got[:, HOLE, 1] == -1)
    assert np.isfinite(want).all() and all(want[:, i].std(axis=0).min() > 0 for i in (0, 1, 3, 4, 5))
    # decisions over all six
    lf.selectLogo()
    best, ratio, text = LS.oracle_decide(orc, want, -1, -1)
    assert lf.getBestLogo() == best == 0
    assert np.float32(lf.getLogoRatio()).tobytes() == ratio.tobytes()
    out = tmp_path / "logof.txt"
    lf.writeResult(out)
    assert out.read_bytes() == text


# ---- 2 ----
@pytest.mark.parametrize("order", ["reversed", "rotated_by_two"])
def test_order_of_the_list_does_not_matter(small, order):
    """The same five logos in another order: every logo's column of records is its column of case 1 (itself the oracle's bytes) -- state
    that is indexed by the wrong logo moves with the order."""
    from amatsukaze_amd import LogoFrame
    perm = [4, 3, 2, 1, 0] if order == "reversed" else [2, 3, 4, 0, 1]
    _, first, _ = small.hole_scan(8, 0)
    lf = LogoFrame(small.ctx, [small.built.logos[p] for p in perm], LS.MASKRATIO)
    got, used = profiled_scan(small.ctx, lf, lambda: lf.scanFrames(small.case(8, 0)["dclip"], batch=17))
    assert used == [PAIR], used
    want = small.want(8, 0)
    for j, p in enumerate(perm):
        assert got[:, j].tobytes() == first[:, p + (p >= HOLE)].tobytes(), (order, "slot", j, "logo", p)
        assert got[:, j].tobytes() == want[:, p].tobytes(), (order, "slot", j, "logo", p)


# ---- 3 ----
def test_two_frames_per_workgroup_ragged_grid(small):
    """1031 frames in one launch: 1031 * 5 / 2048 = 2 frames per workgroup, 516 frame groups of which the last holds one frame; 516 is no
    multiple of the eight groups a block of workgroup ids covers, so four ids per logo leave at once -- with logos whose band counts
    differ."""
    import amt_synth as S
    from amatsukaze_amd import LogoFrame
    W, H = LS.SMALL_FRAME
    N = 1031
    assert N * len(LS.SMALL_MIXED) // 2048 == 2 and N % 2 == 1 and ((N + 1) // 2) % 8 == 4
    alpha, alphaUV = (a.copy() for a in LS.logo_planes(LS.LOGO_A)[1:])        # (shared, read-only arrays: torch wants its own)
    Yd = S.make_clip_torch(N, W, H, 0x5EED0021, alpha, alphaUV, LS.LOGO_A[2], LS.LOGO_A[3], small.gpu["dev"], period=40, fade=6, chroma=False)["Y"]
    lf = LogoFrame(small.ctx, small.built.logos, LS.MASKRATIO)
    lf.begin(W, H, 8, N)
    got, used = profiled_scan(small.ctx, lf, lambda: lf.scan_batch(Yd, 8, 0, N))
    assert used == [PAIR], used
    want = LS.oracle_scan(small.orc, small.built.evals, Yd.cpu().numpy(), 8, LS.SMALL_FRAME)
    for i in range(5):
        assert got[:, i].tobytes() == want[:, i].tobytes(), ("logo", i)
    assert got[N - 1].tobytes() == want[N - 1].tobytes()                 # the group of one frame


# ---- 4 ----
@pytest.mark.parametrize("bits", [8, 10])
def test_wide_mixed_on_the_pair_kernel(gpu, bits):
    """a 680-wide logo (tiles from many column ranges) next to a 36 x 60 and a 130 x 20 one in an 800 x 96 frame"""
    from amatsukaze_amd import LogoFrame
    cs = make_case(gpu, WIDE, bits=bits, pitch_pad=0)
    built = LS.build(LS.WIDE_MIXED, LS.WIDE_FRAME, orc=cs["orc"], ctx=gpu["ctx"])
    lf = LogoFrame(gpu["ctx"], built.logos, LS.MASKRATIO)
    got, used = profiled_scan(gpu["ctx"], lf, lambda: lf.scanFrames(cs["dclip"]))
    assert used == [PAIR], used
    want = LS.oracle_scan(cs["orc"], built.evals, cs["clip"]["Y"], bits, LS.WIDE_FRAME)
    for i in range(3):
        assert got[:, i].tobytes() == want[:, i].tobytes(), ("logo", i)
    assert np.isfinite(want).all()


# ---- 5 ----
def plant_1e31(entry):
    """the entry's planes with one A-plane coefficient of luma (row 2, column 5) at 1e31: bg stays finite, so the oracle's records are
    ordinary numbers, and |a| + |b| >= 8192 keeps the whole list off the pair kernel (test_logoframe_scan_kernel_choice)"""
    data = LS.logo_data(entry).copy()
    data[entry[0] * 2 + 5] = 1e31
    return data


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("which", ["small_1e31_in_C", "small_plus_tiny", "wide_1e31_in_smallest"])
def test_whole_list_on_the_generic_kernel(gpu, small, which, bits):
    """One logo the pair kernel does not take sends every logo of the list to logo_eval_fused_kernel, where all share one LDS plane size
    (the largest band of any logo) while every band has its own row pitch, first column and width: small logos under a large logo's plane,
    and in the 800 x 96 frame whole-row bands (36 and 130 wide) and column bands (680 wide) in one launch."""
    from amatsukaze_amd import LogoFrame
    ctx = gpu["ctx"]
    if which.startswith("small"):
        cs, frame = small.case(bits, 0), LS.SMALL_FRAME
        if which == "small_1e31_in_C":
            entries, planted = LS.SMALL_MIXED, 2
        else:
            entries, planted = LS.SMALL_MIXED + [LS.TINY], None
    else:
        cs, frame = make_case(gpu, WIDE, bits=bits, pitch_pad=0), LS.WIDE_FRAME
        entries = LS.WIDE_MIXED
        planted = min(range(len(entries)), key=lambda i: entries[i][0] * entries[i][1])
        assert entries[planted] == (36, 60, 2, 4)
    data = {planted: plant_1e31(entries[planted])} if planted is not None else None
    built = LS.build(entries, frame, orc=cs["orc"], ctx=ctx, data=data)
    lf = LogoFrame(ctx, built.logos, LS.MASKRATIO)
    got, used = profiled_scan(ctx, lf, lambda: lf.scanFrames(cs["dclip"], batch=17))
    assert used == [GENERIC], used
    want = LS.oracle_scan(cs["orc"], built.evals, cs["clip"]["Y"], bits, frame)
    if planted is not None:
        assert np.isfinite(want[:, planted]).all()
    for i in range(len(entries)):
        assert got[:, i].tobytes() == want[:, i].tobytes(), (which, "logo", i, entries[i])
    assert got.tobytes() == want.tobytes()


# ---- 6 ----
def test_logo_of_another_frame_size_in_the_first_slot(small):
    """[other size, A, B]: the engine's first logo is the list's second; the skipped slot keeps {0, -1}"""
    from amatsukaze_amd import LogoFrame
    W, H = LS.SMALL_FRAME
    cs = small.case(8, 0)
    built = LS.build([LS.LOGO_E, LS.LOGO_A, LS.LOGO_B], LS.SMALL_FRAME, orc=small.orc, ctx=small.ctx, frames={0: (W + 16, H)})
    lf = LogoFrame(small.ctx, built.logos, LS.MASKRATIO)
    got, used = profiled_scan(small.ctx, lf, lambda: lf.scanFrames(cs["dclip"], batch=17))
    assert used == [PAIR], used
    want = LS.oracle_scan(small.orc, built.evals, cs["clip"]["Y"], 8, LS.SMALL_FRAME)
    assert np.all(got[:, 0, 0] == 0) and np.all(got[:, 0, 1] == -1)
    assert got.tobytes() == want.tobytes()
    assert want[:, 1:].tobytes() == small.want(8, 0)[:, :2].tobytes()


# ---- 7 ----
def test_rows_and_columns_of_the_list(small, tmp_path):
    """amtgpu_logoframe_get_rows / _get_columns (include/amt_gpu.h): the union of the rectangles of every logo that was loaded -- what
    the C++ layer uploads.  A logo made for another frame size counts (it was loaded); files that cannot be read do not."""
    from amatsukaze_amd import LogoFrame
    ctx, lib = small.ctx, small.ctx.lib
    W, H = LS.SMALL_FRAME

    def rows_cols(lf):
        r, c = (C.c_int * 2)(7, 7), (C.c_int * 2)(7, 7)
        assert lib.amtgpu_logoframe_get_rows(lf.h, r) == 1 and lib.amtgpu_logoframe_get_columns(lf.h, c) == 1
        return tuple(r), tuple(c)

    p = small.built.paths                                                  # A, B, C, D, E
    assert rows_cols(LogoFrame(ctx, [p[0], p[1], p[3]], LS.MASKRATIO)) == ((18, 240), (6, 352))
    assert rows_cols(LogoFrame(ctx, [p[0], small.missing, p[1]], LS.MASKRATIO)) == ((18, 220), (6, 320))
    other = LS.build([LS.LOGO_C], LS.SMALL_FRAME, ctx=ctx, frames={0: (W + 16, H)}).logos[0]
    lg = small.built.logos
    assert rows_cols(LogoFrame(ctx, [lg[0], lg[1], lg[3], other], LS.MASKRATIO)) == ((0, 240), (6, 352))
    assert rows_cols(LogoFrame(ctx, [small.missing, str(tmp_path / "absent.lgd")], LS.MASKRATIO)) == ((0, 0), (0, 0))
