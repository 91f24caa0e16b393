"""The band cutters of the tile plans (tests/cpp/tile_cut_test.cpp over amatsukaze_amd/csrc/eval_tiles.hpp).

The scan kernel walks a logo band by band and its waves meet once per band, so fewer, fuller bands are less work; its terms are added in
raster order whatever the cut, so its records cannot change.  The finer cut must give plans as valid as the coarse one's, 16 bands
instead of 17 for the bench's main and second candidate logo, no more than 17 for the third, and never a higher modelled critical path
(per band the busiest SIMD's 131 + 31 * passes per tile) than the coarse cut."""
import os
import re
import subprocess

import numpy as np
import pytest

import amtlib
import amt_synth as S

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


# (logo, evaluation logo, bound on the bands of the cut the scan uses; 0: none -- the field logos are not scan logos)
@pytest.mark.parametrize("logo,kind,max_bands", [("main", "deint", 16), ("cand2", "deint", 16), ("cand3", "deint", 17), ("main", "top", 0), ("main", "bottom", 0)])
def test_bench_logo_masks(cut_bin, tmp_path, logo, kind, max_bands):
    """the masks CreateLogoMask (LogoScan.hpp:112-229, through the oracle) gives the bench's logos at its mask ratio"""
    O = amtlib.Oracle()
    hl = O.make_logo(bench_logo(logo), LW, LH, W, H, IMGX, IMGY)
    d = O.lib.orc_logo_deint(hl) if kind == "deint" else O.lib.orc_logo_field(hl, 0 if kind == "top" else 1)
    O.lib.orc_logo_create_mask(d, MASKRATIO, 0)
    info = O.logo_info(d)
    w, h = int(info[0]), int(info[1])
    mask = O.logo_arrays(d)[1].reshape(h, w)
    ys, xs = np.nonzero(mask[2:h - 2, 2:w - 2])
    pos = ((ys + 2).astype(np.uint32) << 16) | (xs + 2).astype(np.uint32)
    fn = tmp_path / "pos.bin"
    with open(fn, "wb") as f:
        np.array([len(pos), w, h], np.int32).tofile(f)
        pos.astype(np.uint32).tofile(f)
    r = subprocess.run([cut_bin, str(fn)] + ([str(max_bands)] if max_bands else []), capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"bands\s+(\d+) /\s+(\d+) /\s+(\d+)\s+modelled critical path\s+(\d+) /\s+(\d+) /\s+(\d+)", r.stdout)
    assert m, r.stdout
    coarse_bands, _, best_bands, coarse_cost, _, best_cost = (int(g) for g in m.groups())
    assert best_cost <= coarse_cost
    if max_bands:
        assert best_bands <= max_bands and coarse_bands == 17        # (17: the parent's cut of these logos)
