"""The scan's one-unit pair kernel (csrc/eval_pair1_kernels.hip) on the smallest shapes at which the form can go wrong, as byte equality of
the scan records with orc_logoframe_scan.

An engine runs the one-unit form when every logo has a single-pass plan that its own model does not price above the best existing cut
(csrc/eval_tiles.hpp tile_plans_single_pass, decided in EvalEngine::ensure_tiles); nothing selects the form from outside and the profile
names the pass, not the form.  So every case states the form its masks lead to, and the host replay (tests/cpp/tile_units_replay.cpp, the
chooser's own code on the masks the oracle gives) confirms it before the records are compared: a case that silently ran the other form
fails there.

  6x6           four pixels, one tile, twelve units
  edge          w % 4 == 2 (130 x 20) flush at the right edge of an unpadded plane: the row's last unit is the one that moves left
  rows          40 x 6 at ratio 1.0: two rows of mask, the unblended first and last row of DeintY in every tile
  sparse        the 130 x 20 logo at ratio 0.02: 52 pixels, tiles that stop at the unit limit far short of 64 pixels, waves without a tile
  full          64 x 24 at ratio 1.0: the units a tile needs are (almost) its box
  at64          LOGO_A (96 x 48) at 0.35: two tiles list exactly 64 units, three stopped where the next pixel by column would have made 65
  three         LOGO_A, the edge logo and LOGO_E in one engine, at 8, 10 and 16 bits and on 1, 8, 9 and 17 frames
  groups        eight frames per workgroup with a last group of one frame (5465 frames x 3 tiny logos)
(the logos of a few rows take tiny_logos.tiny_logo's planes: logo_sets' drawing gives them a black score of zero and records of NaN)
  keeps_old     LOGO_A beside LOGO_B (36 x 100, tall: its single-pass plan costs 1296 against 1158): the engine keeps the parent's plans and
                the two-unit kernel, and LOGO_A's records are the bytes the one-unit form gave
  not_eligible  a 4 x 6 logo in the list: no tile kernel at all, the generic kernel as before
"""
import os
import subprocess

import numpy as np
import pytest

import amtlib
import logo_sets as LS
import tiny_logos as T
from test_gpu_parity import gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PAIR, GENERIC = "logo_eval_pair_kernel.scan", "logo_eval_fused_kernel.scan"
EDGE = (130, 20, 110, 0)                     # in a 240 x 24 frame: ends on the plane's last column
ROWS = (40, 6, 20, 8)
FULL = (64, 24, 8, 4)
SIX = (6, 6, 16, 10)
NFRAMES = 17


@pytest.fixture(scope="module")
def replay_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tile_units") / "tile_units_replay")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(amtlib.ROOT, "amatsukaze_amd", "csrc"),
                           os.path.join(amtlib.ROOT, "tests", "cpp", "tile_units_replay.cpp"), "-o", out])
    return out


def plan_stats(replay_bin, orc, eval_logo, tmp):
    fn = tmp / "pos.bin"
    LS.write_mask_positions(orc, eval_logo, fn)
    r = subprocess.run([replay_bin, str(fn)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    (line,) = [l for l in r.stdout.splitlines() if l.startswith("STATS ")]
    kv = dict(t.split("=", 1) for t in line.split()[1:])
    kv.pop("name")
    return {k: float(v) for k, v in kv.items()}


def noise_clip(n, W, H, bits, seed):
    """(n, H, W) frames, pitch == width: 8 x 8 blocks of every level of the depth (the score bins, both clamps) under fine noise"""
    rng = np.random.default_rng(seed)
    maxv = (1 << bits) - 1
    base = rng.integers(-maxv // 8, maxv + maxv // 8, (n, (H + 7) // 8, (W + 7) // 8)).repeat(8, axis=1).repeat(8, axis=2)[:, :H, :W]
    Y = np.clip(base + rng.integers(-(maxv // 16) - 1, maxv // 16 + 2, (n, H, W)), 0, maxv)
    return np.ascontiguousarray(Y.astype(np.uint8 if bits <= 8 else np.uint16))


def device(gpu, Y):
    return gpu["torch"].from_numpy(Y if Y.dtype == np.uint8 else Y.view(np.int16)).to(gpu["dev"])


def scan(gpu, logos, ratio, Yd, W, H, bits, n=None):
    """-> (records [frames][logos][2], kernels the context launched)"""
    from amatsukaze_amd import LogoFrame
    ctx = gpu["ctx"]
    n = int(Yd.shape[0]) if n is None else n
    lf = LogoFrame(ctx, logos, ratio)
    lf.begin(W, H, bits, n)
    ctx.profile(True)
    try:
        lf.scan_batch(Yd[:n], bits, 0, n)
        got = lf.evalResults
        used = [k for k, (calls, _) in ctx.profile_report().items() if calls]
    finally:
        ctx.profile(False)
    return got, used


def check_form(replay_bin, orc, built, tmp, one_unit, expect=None):
    """the engine's choice for the list, replayed: the one-unit form iff every logo's single-pass plan is no dearer than its best cut"""
    stats = [plan_stats(replay_bin, orc, e, tmp) for e in built.evals]
    assert all(s["single_pass"] == 1 for s in stats) == one_unit, stats
    for s in stats:
        assert s["max_nunits"] <= 64 and s["units_over_need"] == 0
    if expect:
        for k, v in expect.items():
            assert stats[0][k] == v, (k, stats[0][k], v)
    return stats


def tiny_planes(entries):
    return {i: T.tiny_logo(e[0], e[1]) for i, e in enumerate(entries)}


# name: (entries, frame, mask ratio, figures of the first logo's single-pass plan)
SINGLE = {
    "6x6": ([SIX], (48, 32), 1.0, {"px": 4, "units_tiles": 1, "max_nunits": 12}),
    "edge": ([EDGE], (240, 24), LS.MASKRATIO, {"tiles_at_64": 1}),
    "rows": ([ROWS], (80, 24), 1.0, {"px": 72}),
    "sparse": ([EDGE], (240, 24), 0.02, {"px": 52, "units_tiles": 3}),
    "full": ([FULL], (80, 32), 1.0, None),
    "at64": ([LS.LOGO_A], LS.SMALL_FRAME, LS.MASKRATIO, {"tiles_at_64": 2, "tiles_stopped_by_units": 3}),
}


@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("name", sorted(SINGLE))
def test_single_logo(gpu, replay_bin, tmp_path, name, bits):
    entries, (W, H), ratio, expect = SINGLE[name]
    orc = amtlib.Oracle()
    built = LS.build(entries, (W, H), orc=orc, ctx=gpu["ctx"], maskratio=ratio, data=tiny_planes(entries) if name in ("6x6", "rows") else None)
    stats = check_form(replay_bin, orc, built, tmp_path, True, expect)
    if name == "full":
        assert stats[0]["units_need"] > 0.95 * stats[0]["units_box"]
    Y = noise_clip(9, W, H, bits, 0x5CA70000 + bits + 31 * sorted(SINGLE).index(name))
    got, used = scan(gpu, built.logos, ratio, device(gpu, Y), W, H, bits)
    assert used == [PAIR], used
    want = LS.oracle_scan(orc, built.evals, Y, bits, (W, H))
    assert np.isfinite(want).all() and want.std() > 0
    assert got.tobytes() == want.tobytes()


class Three:
    """LOGO_A, the w % 4 == 2 logo on the frame's last column and LOGO_E in one engine: clips and the oracle's records per depth, once"""
    ENTRIES = [LS.LOGO_A, (130, 20, 222, 100), LS.LOGO_E]

    def __init__(self, gpu):
        self.gpu, self.orc = gpu, amtlib.Oracle()
        self.built = LS.build(self.ENTRIES, LS.SMALL_FRAME, orc=self.orc, ctx=gpu["ctx"])
        self._clips = {}

    def clip(self, bits):
        if bits not in self._clips:
            W, H = LS.SMALL_FRAME
            Y = noise_clip(NFRAMES, W, H, bits, 0x5CA71000 + bits)
            want = LS.oracle_scan(self.orc, self.built.evals, Y, bits, LS.SMALL_FRAME)
            Y.setflags(write=False); want.setflags(write=False)
            self._clips[bits] = (Y, device(self.gpu, np.array(Y)), want)
        return self._clips[bits]


@pytest.fixture(scope="module")
def three(gpu):
    return Three(gpu)


@pytest.mark.parametrize("bits,n", [(8, 1), (8, 8), (8, 9), (8, 17), (10, 17), (16, 17)])
def test_three_logos_of_different_sizes(gpu, three, replay_bin, tmp_path, bits, n):
    assert Three.ENTRIES[1][2] + Three.ENTRIES[1][0] == LS.SMALL_FRAME[0] and Three.ENTRIES[1][0] % 4 == 2
    check_form(replay_bin, three.orc, three.built, tmp_path, True)
    Y, Yd, want = three.clip(bits)
    got, used = scan(gpu, three.built.logos, LS.MASKRATIO, Yd, *LS.SMALL_FRAME, bits, n=n)
    assert used == [PAIR], used
    for i in range(3):
        assert got[:, i].tobytes() == want[:n, i].tobytes(), ("logo", i)
    assert np.isfinite(want).all()


def test_eight_frames_per_workgroup_last_group_of_one(gpu, replay_bin, tmp_path):
    """5465 frames x 3 logos: 5465 * 3 / 2048 = 8 frames per workgroup, 684 groups of which the last holds one frame"""
    N, (W, H) = 5465, (64, 32)
    assert N * 3 // 2048 == 8 and N % 8 == 1
    entries = [SIX, (40, 6, 20, 20), (22, 12, 40, 2)]
    orc = amtlib.Oracle()
    built = LS.build(entries, (W, H), orc=orc, ctx=gpu["ctx"], maskratio=1.0, data=tiny_planes(entries))
    stats = check_form(replay_bin, orc, built, tmp_path, True)
    assert [s["px"] for s in stats] == [4, 72, 144]
    Y = noise_clip(N, W, H, 8, 0x5CA72000)
    got, used = scan(gpu, built.logos, 1.0, device(gpu, Y), W, H, 8)
    assert used == [PAIR], used
    want = LS.oracle_scan(orc, built.evals, Y, 8, (W, H))
    assert np.isfinite(want).all()
    for i in range(3):
        assert got[:, i].tobytes() == want[:, i].tobytes(), ("logo", i)
    assert got[N - 1].tobytes() == want[N - 1].tobytes()


@pytest.mark.parametrize("bits", [8, 10])
def test_a_logo_that_keeps_the_old_form(gpu, three, replay_bin, tmp_path, bits):
    """LOGO_B's tiles are tall: under the unit limit it needs 27 tiles in 3 bands instead of 20 in 2, and the model prices that above the
    second passes it saves.  The engine of [LOGO_A, LOGO_B] keeps the two-unit kernel on the parent's plans; LOGO_A's records there are
    the bytes of the one-unit engines (the oracle's)."""
    orc = three.orc
    built = LS.build([LS.LOGO_A, LS.LOGO_B], LS.SMALL_FRAME, orc=orc, ctx=gpu["ctx"])
    stats = check_form(replay_bin, orc, built, tmp_path, False)
    assert stats[0]["single_pass"] == 1 and stats[1]["single_pass"] == 0
    assert stats[1]["units_cost"] > min(stats[1]["coarse_cost"], stats[1]["fine_cost"])
    Y, Yd, want3 = three.clip(bits)
    got, used = scan(gpu, built.logos, LS.MASKRATIO, Yd, *LS.SMALL_FRAME, bits)
    assert used == [PAIR], used
    want = LS.oracle_scan(orc, built.evals, np.array(Y), bits, LS.SMALL_FRAME)
    assert got.tobytes() == want.tobytes()
    assert got[:, 0].tobytes() == want3[:, 0].tobytes()
    alone, used = scan(gpu, built.logos[:1], LS.MASKRATIO, Yd, *LS.SMALL_FRAME, bits)      # the one-unit form on the same clip
    assert used == [PAIR] and alone[:, 0].tobytes() == got[:, 0].tobytes()


def test_a_logo_no_tile_kernel_takes(gpu, three):
    """a 4 x 6 logo in the list sends every logo to the generic kernel, as before"""
    orc = three.orc
    built = LS.build([LS.LOGO_A, LS.TINY], LS.SMALL_FRAME, orc=orc, ctx=gpu["ctx"])
    Y, Yd, want3 = three.clip(8)
    got, used = scan(gpu, built.logos, LS.MASKRATIO, Yd, *LS.SMALL_FRAME, 8)
    assert used == [GENERIC], used
    want = LS.oracle_scan(orc, built.evals, np.array(Y), 8, LS.SMALL_FRAME)
    assert got[:, 0].tobytes() == want[:, 0].tobytes() == want3[:, 0].tobytes()
    assert got.tobytes() == want.tobytes()
