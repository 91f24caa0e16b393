"""CPU replay of the single-pass tile plans (tests/cpp/tile_units_replay.cpp over amatsukaze_amd/csrc/eval_tiles.hpp, kTileCutUnits): the
plans the scan's one-unit pair kernel runs on.  The program checks every plan it builds -- slots, bands, unit lists, windows against
the staged cells -- and prints one STATS line per mask with the figures of the existing cuts beside the single-pass plan's; the tests
here feed it the masks tests/test_eval_tiles.py uses and pin the bench logo's figures.

Which of these masks make the engine's chooser keep the two-unit form (single_pass=0 on the STATS line: the single-pass plan's modelled
cost is above the best existing cut's) is recorded in profiles/scan_units_notes.md; test_masks_that_keep_the_old_form pins the seeded ones.
"""
import os
import subprocess

import pytest

import amtlib
import amt_synth as S
from logo_sets import REPLAY_CASES, REPLAY_IDS, logo_data, oracle_eval_logo, write_mask_positions

ROOT = amtlib.ROOT


@pytest.fixture(scope="module")
def replay_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tile_units") / "tile_units_replay")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "amatsukaze_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "tile_units_replay.cpp"), "-o", out])
    return out


def run_replay(replay_bin, *args):
    """-> {mask name: {figure: value}} of the STATS lines; the program's own checks must all have passed"""
    r = subprocess.run([replay_bin, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        if not line.startswith("STATS "):
            continue
        kv = dict(t.split("=", 1) for t in line.split()[1:])
        name = kv.pop("name")
        out[name] = {k: float(v) for k, v in kv.items()}
    assert out, r.stdout
    return out


def test_seeded_masks(replay_bin):
    stats = run_replay(replay_bin)
    print({k: (v["units_cost"], min(v["coarse_cost"], v["fine_cost"]), v["single_pass"]) for k, v in stats.items()})
    for name, s in stats.items():
        assert s["units_over_need"] == 0 and s["max_nunits"] <= 64, name
    # a full mask: a window's units are the box's, the rule changes next to nothing
    assert stats["full-64x24"]["units_need"] == stats["full-64x24"]["coarse_need"]
    # tiles with exactly 64 needed units, next to tiles the unit limit stopped (the next pixel by column would have made 65 or more)
    assert stats["random-60%-90x33"]["tiles_at_64"] >= 1 and stats["random-60%-90x33"]["tiles_stopped_by_units"] >= 1


def test_masks_that_keep_the_old_form(replay_bin):
    """dense random masks and tall or wide ones need more than 64 units per 64 pixels: forcing their tiles under the limit costs more tiles
    than it saves passes, and the chooser keeps the existing plans"""
    stats = run_replay(replay_bin)
    keep = sorted(k for k, v in stats.items() if not v["single_pass"])
    assert keep == sorted(["random-35%-256x128", "strokes-256x128", "columns-256x128", "wide-1022x40", "tall-22x400", "narrow-6x200",
                           "w%4==2-66x50", "random-10%-130x20"])
    for k in keep:
        assert stats[k]["units_cost"] > min(stats[k]["coarse_cost"], stats[k]["fine_cost"])


def within(v, lo, hi, digits):
    """v lies in [lo, hi] as a table rounded to `digits` decimals states it"""
    return round(v, digits) >= lo and round(v, digits) <= hi


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
    (s,) = run_replay(replay_bin, str(fn)).values()
    print(kind, ratio, s)
    if ratio != 0.35:
        return
    # the single-pass plan is modelled cheaper than the best existing cut, and the chooser takes it
    assert s["units_cost"] < min(s["coarse_cost"], s["fine_cost"]) and s["single_pass"] == 1
    if kind == "deint":
        # the bench's main logo: the existing cuts ...
        for cut in ("coarse", "fine"):
            assert 174 <= s[cut + "_tiles"] <= 179
            assert within(s[cut + "_box"], 65.4, 67.5, 1) and within(s[cut + "_need"], 53.2, 53.6, 1)
            assert within(s[cut + "_over_box"], 42, 45, 0) and within(s[cut + "_over_need"], 15, 16, 0)
        # ... and 174 tiles in 16 bands at 8 458 against 177 in 17 at 7 938
        best = "fine" if s["fine_cost"] < s["coarse_cost"] else "coarse"
        assert (s[best + "_tiles"], s[best + "_bands"], s[best + "_cost"]) == (174, 16, 8458)
        assert (s["units_tiles"], s["units_bands"], s["units_cost"]) == (177, 17, 7938)
    else:
        for cut in ("coarse", "fine"):
            assert 82 <= s[cut + "_tiles"] <= 85
            assert within(s[cut + "_box"], 69.5, 70.5, 1) and within(s[cut + "_need"], 54.3, 56.2, 1)
            assert within(s[cut + "_over_box"], 52, 55, 0) and within(s[cut + "_over_need"], 18, 21, 0)


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
    (s,) = run_replay(replay_bin, str(fn)).values()
    print(entry, ratio, s)
    if (w, h) == (6, 6):
        assert count == 4 and s["units_tiles"] == 1 and s["max_nunits"] == 12
