"""The scan pair kernel's second shape (csrc/eval_pair1_duo_kernels.hip: 7 evaluation waves + the summing wave, at most 6 frames per
workgroup, two workgroups per CU) as byte equality of the scan records with orc_logoframe_scan.

An engine takes the shape when tile_pair_shape (csrc/eval_tiles.hpp, decided in EvalEngine::ensure_tiles) says so; nothing selects it from
outside and the profile names the pass, not the form.  So every case first replays the choice for its logo list on the host
(tests/cpp/pair_shape_replay.cpp through tests/test_pair_shape.py, which pins the same verdicts without a GPU) and asserts the form it is
about; a case that silently ran another form fails there.

  six           6 x 6, four pixels, one tile: six of the seven evaluation waves idle through every barrier
  full          64 x 24 at ratio 1.0: bands of exactly seven tiles followed by one of five
  three         LOGO_A, a w % 4 == 2 logo on the frame's last column and LOGO_E in one engine, on 1, 5, 6, 7 and 13 frames -- ONE frame per
                workgroup at these counts (the engine's rule: frames x logos / 2048), so they are 1 to 13 groups in grids of 8 and 16, not
                a workgroup's boundaries: tiny3 has those -- and at 8, 10 and 16 bits
  tiny3         4 098, 4 099, 4 103 and 4 104 frames x 3 tiny logos: six frames per workgroup -- the shape's most -- in whole groups and
                with a last group of one and of five frames
  keeps_old     the 680-wide logo of WIDE_MIXED keeps the two-unit form: the engine runs the parent's two-unit kernel on the parent's plans
  keeps_eleven  LOGO_D beside LOGO_A: 81 tiles at seven per band against 80 -- the one-unit kernel at 11 + 1, as in the parent
"""
import numpy as np
import pytest

import amtlib
import logo_sets as LS
import test_pair_shape as PS
from test_gpu_parity import gpu  # noqa: F401  (fixture)
from test_gpu_scan_units import PAIR, device, noise_clip, scan
from test_pair_shape import replay_bin  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


class Case:
    """one logo list in every form, its replayed verdict, and per depth a clip with the oracle's records -- built once"""

    def __init__(self, gpu, replay_bin, tmp, name):
        self.gpu, self.name, self.orc = gpu, name, amtlib.Oracle()
        self.frame, self.ratio = PS.LISTS[name][1], PS.LISTS[name][2]
        self.built = PS.build_list(name, self.orc, gpu["ctx"])
        # the replay decides with the limit the engine queries (hipDeviceAttributeMaxSharedMemoryPerBlock is the device property torch
        # reports): a device whose limit sent the engine to the 11 + 1 kernels fails the case's form here instead of passing on them
        lds = int(gpu["torch"].cuda.get_device_properties(gpu["dev"]).shared_memory_per_block)
        self.plans, self.choice = PS.verdict(replay_bin, self.orc, self.built.evals, tmp, "--lds", str(lds))
        assert self.choice["lds_limit"] == lds and lds >= PS.DUO_LDS, (lds, self.choice)
        assert self.choice["waves"] == PS.LISTS[name][4], self.choice
        self._clips = {}

    def duo(self):
        return self.choice["duo"] == 1 and self.choice["waves"] == PS.DUO_WAVES and self.choice["frames"] == PS.DUO_FRAMES

    def clip(self, bits, n):
        if (bits, n) not in self._clips:
            W, H = self.frame
            Y = noise_clip(n, W, H, bits, 0x5CA73000 + bits + 64 * sorted(PS.LISTS).index(self.name))
            want = LS.oracle_scan(self.orc, self.built.evals, Y, bits, self.frame)
            assert np.isfinite(want).all() and want.std() > 0
            Y.setflags(write=False); want.setflags(write=False)
            self._clips[bits, n] = (device(self.gpu, np.array(Y)), want)
        return self._clips[bits, n]

    def check(self, bits, nclip, n=None):
        n = nclip if n is None else n
        Yd, want = self.clip(bits, nclip)
        got, used = scan(self.gpu, self.built.logos, self.ratio, Yd, *self.frame, bits, n=n)
        assert used == [PAIR], used
        for i in range(len(self.built.logos)):
            assert got[:, i].tobytes() == want[:n, i].tobytes(), ("logo", i)


_cases = {}


@pytest.fixture
def case(gpu, replay_bin, tmp_path_factory):
    def get(name):
        if name not in _cases:
            _cases[name] = Case(gpu, replay_bin, tmp_path_factory.mktemp("scan_waves_" + name), name)
        return _cases[name]
    return get


@pytest.mark.parametrize("bits", [8, 10, 16])
def test_one_tile_logo(case, bits):
    c = case("six")
    assert c.duo() and c.plans[0]["px"] == 4 and c.plans[0]["duo_tiles_per_band"] == [1]
    c.check(bits, 9)


@pytest.mark.parametrize("bits", [8, 10, 16])
def test_a_band_of_seven_tiles_then_a_shorter_one(case, bits):
    c = case("full")
    t = c.plans[0]["duo_tiles_per_band"]
    assert c.duo() and any(a == PS.DUO_WAVES and b < PS.DUO_WAVES for a, b in zip(t, t[1:])), t
    c.check(bits, 9)


@pytest.mark.parametrize("bits,n", [(8, 1), (8, 5), (8, 6), (8, 7), (8, 13), (10, 13), (16, 13)])
def test_three_logos_of_different_sizes(case, bits, n):
    c = case("three")
    assert c.duo() and len({(p["px"], p["duo_bands"]) for p in c.plans}) >= 2
    c.check(bits, 13, n)


@pytest.mark.parametrize("n", [4098, 4099, 4103, 4104])
def test_six_frames_per_workgroup(case, n):
    """3 logos x n frames with n * 3 / 2048 = 6: six frames per workgroup, the shape's most (the parent's rule gives 6 here as well).
    4 098 and 4 104 are whole groups (683, 684), 4 099 leaves a last group of one frame, 4 103 one of G - 1 = 5; the counts are the first
    n frames of one clip of 4 104"""
    G = PS.DUO_FRAMES
    assert n * 3 // 2048 == G and {m: m % G for m in (4098, 4099, 4103, 4104)} == {4098: 0, 4099: 1, 4103: G - 1, 4104: 0}
    c = case("tiny3")
    assert c.duo() and [p["px"] for p in c.plans] == [4, 72, 144]
    c.check(8, 4104, n)


@pytest.mark.parametrize("name", ["keeps_old", "keeps_eleven"])
def test_a_list_that_keeps_the_parents_kernels(case, name):
    c = case(name)
    assert not c.duo() and (c.choice["waves"], c.choice["frames"]) == (PS.WAVES, PS.FRAMES)
    assert c.choice["one_unit"] == (1 if name == "keeps_eleven" else 0)
    c.check(8, 9)
