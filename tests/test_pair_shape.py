"""CPU replay of the scan pair kernel's shape choice (tests/cpp/pair_shape_replay.cpp over amatsukaze_amd/csrc/eval_tiles.hpp): the plans of
seven tiles per band that the kernel's second shape walks (csrc/eval_pair1_duo_kernels.hip: 7 + 1 waves, two workgroups per CU), built
through build_tile_plan's trailing wave-count argument, and tile_pair_shape, the pure function EvalEngine::ensure_tiles decides with.

The program checks every plan it builds (its header lists what) and that the argument at its default changes no byte of any cut; the tests
feed it the masks tests/test_eval_tiles.py uses and every logo list tests/test_gpu_scan_waves.py scans, and pin the verdicts: that file
imports LISTS and `verdict` from here, so the form a GPU case states is the one replayed here without a GPU.
"""
import os
import subprocess

import pytest

import amtlib
import amt_synth as S
import logo_sets as LS
import tiny_logos as T

ROOT = amtlib.ROOT
DUO_WAVES, DUO_FRAMES, WAVES, FRAMES = 7, 6, 11, 8
DUO_LDS = 7 * 4096 + 2 * 2 * 6 * (7 * 64 + 36) * 4          # planes + two sets of 2 G score rows (csrc/eval_tiles.hpp tile_pair_lds_bytes)

SIX = (6, 6, 16, 10)
FULL = (64, 24, 8, 4)
THREE = [LS.LOGO_A, (130, 20, 222, 100), LS.LOGO_E]
TINY3 = [SIX, (40, 6, 20, 20), (22, 12, 40, 2)]
# name: (entries, frame, mask ratio, tiny_logos planes, the replayed verdict: evaluation waves)
LISTS = {
    "six": ([SIX], (48, 32), 1.0, True, DUO_WAVES),
    "full": ([FULL], (80, 32), 1.0, False, DUO_WAVES),
    "three": (THREE, LS.SMALL_FRAME, LS.MASKRATIO, False, DUO_WAVES),
    "tiny3": (TINY3, (64, 32), 1.0, True, DUO_WAVES),
    "keeps_old": (LS.WIDE_MIXED, LS.WIDE_FRAME, LS.MASKRATIO, False, WAVES),                      # ... and the two-unit form
    "keeps_eleven": ([LS.LOGO_A, LS.LOGO_D], LS.SMALL_FRAME, LS.MASKRATIO, False, WAVES),       # ... the one-unit form at 11 + 1
}


def build_replay(tmp, flags=("-O2",)):
    out = str(tmp / "pair_shape_replay")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "amatsukaze_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "pair_shape_replay.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def replay_bin(tmp_path_factory):
    return build_replay(tmp_path_factory.mktemp("pair_shape"))


def run_replay(replay_bin, *args):
    """-> ([{figure: value} per PLAN line], [{...} per CHOICE line]); the program's own checks must all have passed"""
    r = subprocess.run([replay_bin, *args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    plans, choices = [], []
    for line in r.stdout.splitlines():
        tag, _, rest = line.partition(" ")
        if tag in ("PLAN", "CHOICE"):
            kv = dict(t.split("=", 1) for t in rest.split(" name=")[0].split())
            if tag == "PLAN":
                kv["name"] = rest.split(" name=")[1]
                kv["duo_tiles_per_band"] = [int(t) for t in kv["duo_tiles_per_band"].split(",")] if kv["duo_tiles_per_band"] != "-" else []
            (plans if tag == "PLAN" else choices).append({k: (int(v) if isinstance(v, str) and v.lstrip("-").isdigit() else v) for k, v in kv.items()})
    return plans, choices


def verdict(replay_bin, orc, evals, tmp, *args):
    """the replayed choice for one engine's list of masked oracle logos -> (plans, choice)"""
    files = []
    for i, e in enumerate(evals):
        files.append(str(tmp / f"pos{i}.bin"))
        LS.write_mask_positions(orc, e, files[-1])
    plans, (choice,) = run_replay(replay_bin, *args, *files)
    assert len(plans) == len(evals) and choice["logos"] == len(evals)
    return plans, choice


def build_list(name, orc, ctx=None):
    entries, frame, ratio, tiny, _ = LISTS[name]
    data = {i: T.tiny_logo(e[0], e[1]) for i, e in enumerate(entries)} if tiny else None
    return LS.build(entries, frame, orc=orc, ctx=ctx, maskratio=ratio, data=data)


def test_seeded_masks(replay_bin):
    """every check of the program on the seeded masks of tile_units_replay.cpp, each an engine of its own; masks whose tiles the unit limit
    multiplies keep the 11 + 1 shape, as they keep the two-unit form"""
    plans, choices = run_replay(replay_bin)
    assert len(plans) == len(choices) == 15
    got = {p["name"]: c["waves"] for p, c in zip(plans, choices)}
    print(got)
    assert all(max(p["duo_tiles_per_band"]) <= DUO_WAVES for p in plans)
    keep = sorted(k for k, v in got.items() if v == WAVES)
    assert keep == sorted(["random-35%-256x128", "strokes-256x128", "wide-1022x40", "narrow-6x200", "w%4==2-66x50", "random-10%-130x20"])
    for p, c in zip(plans, choices):
        existing = min(p["best_cost"], p["units_cost"])
        assert (c["waves"] == DUO_WAVES) == ((p["duo_work"] + 3) // 4 <= existing), p
        assert (c["waves"], c["frames"]) in ((DUO_WAVES, DUO_FRAMES), (WAVES, FRAMES))
        if c["waves"] == DUO_WAVES:
            assert c["lds"] == DUO_LDS == 75136 and c["one_unit"] == 1


@pytest.mark.parametrize("kind,ratio", [("deint", 0.35), ("field", 0.35), ("deint", 0.1), ("deint", 1.0)])
def test_bench_logo_masks(replay_bin, tmp_path, kind, ratio):
    """the masks CreateLogoMask (through the oracle) gives the bench logo"""
    O = amtlib.Oracle()
    data, _, _ = S.make_logo(256, 128)
    hl = O.make_logo(data, 256, 128, 1440, 1080, 1120, 64)
    d = O.lib.orc_logo_deint(hl) if kind == "deint" else O.lib.orc_logo_field(hl, 0)
    O.lib.orc_logo_create_mask(d, ratio, 0)
    (p,), c = verdict(replay_bin, O, [d], tmp_path)
    print(kind, ratio, p, c)
    if (kind, ratio) == ("deint", 0.35):
        # the bench's main logo: 183 tiles in 27 bands against 177 in 17; 183 * 162 / 4 = 7 412 against 7 938
        assert (sum(p["duo_tiles_per_band"]), p["duo_bands"], p["duo_work"], p["units_cost"]) == (183, 27, 183 * 162, 7938)
        assert c["waves"] == DUO_WAVES and c["frames"] == DUO_FRAMES


def test_bench_logo_list(replay_bin, tmp_path):
    """the three logos bench.py scans, as one engine: the second shape; and the parent's shape where a workgroup's LDS does not fit"""
    import bench
    O = amtlib.Oracle()
    logos_np, _, _ = bench.make_logos()
    evals = [LS.oracle_eval_logo(O, O.make_logo(d, bench.LW, bench.LH, 1440, 1080, 1120, 64)) for d in logos_np]
    plans, c = verdict(replay_bin, O, evals, tmp_path)
    print(plans, c)
    assert (c["waves"], c["frames"], c["one_unit"], c["lds"]) == (DUO_WAVES, DUO_FRAMES, 1, DUO_LDS)
    _, c64 = verdict(replay_bin, O, evals, tmp_path, "--lds", "65536")
    assert (c64["waves"], c64["frames"], c64["one_unit"]) == (WAVES, FRAMES, 1)
    _, cfit = verdict(replay_bin, O, evals, tmp_path, "--lds", str(DUO_LDS))
    assert cfit["waves"] == DUO_WAVES


@pytest.mark.parametrize("entry,ratio", LS.REPLAY_CASES, ids=LS.REPLAY_IDS)
def test_mixed_logo_masks(replay_bin, tmp_path, entry, ratio):
    """the masks of every logo the mixed-list scans run (tests/logo_sets.py), each an engine of its own"""
    O = amtlib.Oracle()
    w, h, imgx, imgy = entry
    d = LS.oracle_eval_logo(O, O.make_logo(LS.logo_data(entry), w, h, imgx + w, imgy + h, imgx, imgy), ratio)
    (p,), c = verdict(replay_bin, O, [d], tmp_path)
    print(entry, ratio, p, c)
    assert p["px"] > 0 and max(p["duo_tiles_per_band"]) <= DUO_WAVES
    if (w, h) == (6, 6):
        assert p["px"] == 4 and p["duo_tiles_per_band"] == [1] and c["waves"] == DUO_WAVES


@pytest.mark.parametrize("name", sorted(LISTS))
def test_gpu_case_lists(replay_bin, tmp_path, name):
    """the verdict for every logo list tests/test_gpu_scan_waves.py scans"""
    O = amtlib.Oracle()
    built = build_list(name, O)
    plans, c = verdict(replay_bin, O, built.evals, tmp_path)
    print(name, plans, c)
    assert c["waves"] == LISTS[name][4]
    if name == "six":
        assert plans[0]["duo_tiles_per_band"] == [1]
    if name == "full":
        # a band of exactly seven tiles followed by a shorter one
        t = plans[0]["duo_tiles_per_band"]
        assert any(a == DUO_WAVES and b < DUO_WAVES for a, b in zip(t, t[1:])), t
    if name == "keeps_old":
        # the 680-wide logo's plans under the unit limit are dearer than its best cut, even spread over four SIMDs: the two-unit kernel
        # on the parent's plans; the other two alone would take the second shape
        w, a, b = plans
        assert (w["duo_work"] + 3) // 4 > w["best_cost"] and w["units_cost"] > w["best_cost"] and c["one_unit"] == 0
        assert all((p["duo_work"] + 3) // 4 <= min(p["best_cost"], p["units_cost"]) for p in (a, b))
    if name == "keeps_eleven":
        # LOGO_D: 81 tiles at seven per band against 80 at eleven -- 3 281 against 3 240; the one-unit kernel at 11 + 1 as in the parent
        a, d = plans
        assert (a["duo_work"] + 3) // 4 <= a["units_cost"] and ((d["duo_work"] + 3) // 4, d["units_cost"]) == (3281, 3240) and c["one_unit"] == 1


def test_sanitized_program_runs_standalone(tmp_path):
    """the program built with -fsanitize=address,undefined and run on its own (no interpreter loads it)"""
    exe = build_replay(tmp_path, ("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    O = amtlib.Oracle()
    for name in ("six", "three"):                     # (the seeded masks take most of a minute under the sanitizers)
        plans, c = verdict(exe, O, build_list(name, O).evals, tmp_path)
        assert c["waves"] == LISTS[name][4] and len(plans) == len(LISTS[name][0])
