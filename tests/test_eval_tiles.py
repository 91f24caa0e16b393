"""CPU replay of the tile kernel's addressing (tests/cpp/eval_tiles_test.cpp over amatsukaze_amd/csrc/eval_tiles.hpp):
every mask pixel's 5x5 window must read the samples CalcCorrelation5x5 reads (LogoScan.hpp:24-41), once, in raster order."""
import os
import subprocess

import pytest

import amtlib
import amt_synth as S
from logo_sets import REPLAY_CASES, REPLAY_IDS, logo_data, oracle_eval_logo, write_mask_positions

ROOT = amtlib.ROOT


@pytest.fixture(scope="module")
def replay_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tiles") / "eval_tiles_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "amatsukaze_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "eval_tiles_test.cpp"), "-o", out])
    return out


def test_synthetic_masks(replay_bin):
    r = subprocess.run([replay_bin], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("kind,ratio", [("deint", 0.35), ("field", 0.35), ("deint", 0.1), ("deint", 1.0)])
def test_bench_logo_masks(replay_bin, tmp_path, kind, ratio):
    """the masks CreateLogoMask (LogoScan.hpp:112-229, through the oracle) gives the bench logo"""
    O = amtlib.Oracle()
    data, _, _ = S.make_logo(256, 128)
    hl = O.make_logo(data, 256, 128, 1440, 1080, 1120, 64)
    d = O.lib.orc_logo_deint(hl) if kind == "deint" else O.lib.orc_logo_field(hl, 0)
    O.lib.orc_logo_create_mask(d, ratio, 0)
    fn = tmp_path / "pos.bin"
    write_mask_positions(O, d, fn)
    r = subprocess.run([replay_bin, str(fn)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("entry,ratio", REPLAY_CASES, ids=REPLAY_IDS)
def test_mixed_logo_masks(replay_bin, tmp_path, entry, ratio):
    """the masks of every logo the mixed-list scans run (tests/logo_sets.py): widths that are no multiple of 4, a tall narrow and a
    680-wide logo, the smallest logo the plans take and a sparse mask"""
    O = amtlib.Oracle()
    w, h, imgx, imgy = entry
    d = oracle_eval_logo(O, O.make_logo(logo_data(entry), w, h, imgx + w, imgy + h, imgx, imgy), ratio)
    fn = tmp_path / "pos.bin"
    count, mw, mh = write_mask_positions(O, d, fn)
    assert (mw, mh) == (w, h) and count > 0
    if (w, h) == (6, 6):
        assert count == 4                        # every pixel is in the mask; four have a window inside the logo
    r = subprocess.run([replay_bin, str(fn)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
