"""The band cutters of the tile plans (tests/cpp/tile_cut_test.cpp over amatsukaze_amd/csrc/eval_tiles.hpp).

The scan kernel walks a logo band by band and its waves meet once per band, so fewer, fuller bands are less work; its terms are added in
raster order whatever the cut, so its records cannot change.  The finer cut must give plans as valid as the coarse one's, 16 bands
instead of 17 for the bench's main and second candidate logo, no more than 17 for the third, and never a higher modelled critical path
(per band the busiest SIMD's 131 + 31 * passes per tile) than the coarse cut."""
import os
import re
import subprocess

import pytest

import amtlib
import amt_synth as S
from logo_sets import REPLAY_CASES, REPLAY_IDS, logo_data, oracle_eval_logo, write_mask_positions

ROOT = amtlib.ROOT
LW, LH, W, H, IMGX, IMGY, MASKRATIO = 256, 128, 1440, 1080, 1120, 64, 0.35      # bench.py's logo, frame and mask ratio


@pytest.fixture(scope="module")
def cut_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tilecut") / "tile_cut_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "amatsukaze_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "tile_cut_test.cpp"), "-o", out])
    return out


def test_synthetic_masks(cut_bin):
    r = subprocess.run([cut_bin], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def bench_logo(name):
    """bench.py make_logos()"""
    if name == "main":
        return S.make_logo(LW, LH)[0]
    return S.make_logo(LW, LH, seed={"cand2": 0x10600002, "cand3": 0x10600003}[name], strength={"cand2": 0.5, "cand3": 0.8}[name])[0]


def cut_figures(stdout):
    """(coarse bands, best bands, coarse cost, best cost) from the program's report"""
    m = re.search(r"bands\s+(\d+) /\s+(\d+) /\s+(\d+)\s+modelled critical path\s+(\d+) /\s+(\d+) /\s+(\d+)", stdout)
    assert m, stdout
    coarse_bands, _, best_bands, coarse_cost, _, best_cost = (int(g) for g in m.groups())
    return coarse_bands, best_bands, coarse_cost, best_cost


# (logo, evaluation logo, bound on the bands of the cut the scan uses; 0: none -- the field logos are not scan logos)
@pytest.mark.parametrize("logo,kind,max_bands", [("main", "deint", 16), ("cand2", "deint", 16), ("cand3", "deint", 17), ("main", "top", 0), ("main", "bottom", 0)])
def test_bench_logo_masks(cut_bin, tmp_path, logo, kind, max_bands):
    """the masks CreateLogoMask (LogoScan.hpp:112-229, through the oracle) gives the bench's logos at its mask ratio"""
    O = amtlib.Oracle()
    hl = O.make_logo(bench_logo(logo), LW, LH, W, H, IMGX, IMGY)
    d = O.lib.orc_logo_deint(hl) if kind == "deint" else O.lib.orc_logo_field(hl, 0 if kind == "top" else 1)
    O.lib.orc_logo_create_mask(d, MASKRATIO, 0)
    fn = tmp_path / "pos.bin"
    write_mask_positions(O, d, fn)
    r = subprocess.run([cut_bin, str(fn)] + ([str(max_bands)] if max_bands else []), capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    coarse_bands, best_bands, coarse_cost, best_cost = cut_figures(r.stdout)
    assert best_cost <= coarse_cost
    if max_bands:
        assert best_bands <= max_bands and coarse_bands == 17        # (17: the parent's cut of these logos)


@pytest.mark.parametrize("entry,ratio", REPLAY_CASES, ids=REPLAY_IDS)
def test_mixed_logo_masks(cut_bin, tmp_path, entry, ratio):
    """the masks of every logo the mixed-list scans run (tests/logo_sets.py): both cuts give valid plans (the program's exit status) and the
    finer one never a higher modelled critical path"""
    O = amtlib.Oracle()
    w, h, imgx, imgy = entry
    d = oracle_eval_logo(O, O.make_logo(logo_data(entry), w, h, imgx + w, imgy + h, imgx, imgy), ratio)
    fn = tmp_path / "pos.bin"
    assert write_mask_positions(O, d, fn)[0] > 0
    r = subprocess.run([cut_bin, str(fn)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    _, _, coarse_cost, best_cost = cut_figures(r.stdout)
    assert best_cost <= coarse_cost
