"""The operand limits of the tile kernels' 24-bit multiplies (tests/cpp/tile_mul24_test.cpp over amatsukaze_amd/csrc/eval_tiles.hpp).

The scan (pair) kernel and the linear analysis kernel form a new tile's offsets -- unit -> row, row x pitch, row x logo width -- with
v_mul_u32_u24, which multiplies the low 24 bits of its operands.  The kernels do not check anything; the host does, where it chooses
them (EvalEngine::pair_addressable -> tile_mul24_operands_ok, ensure_tiles -> tile_slots_ok), and keeps the generic kernel otherwise.
The program checks those functions at their limits (pitch 2^24 - 1 / 2^24 / 2^24 + 1 bytes, row 2^24 - 1 / 2^24, 2^20 - 1 / 2^20
slots), replays the instruction's arithmetic against plain multiplication over everything they admit -- every staging unit of every
tile shape, two million random (pitch, row, logo row, width) -- and shows that one operand at 2^24 already gives another result.
tests/cpp/eval_tiles_test.cpp (test_eval_tiles.py) replays the same header's addressing on whole tile plans, unchanged."""
import os
import subprocess

import amtlib

ROOT = amtlib.ROOT


def test_guard_limits_and_device_multiply_replay(tmp_path):
    out = str(tmp_path / "tile_mul24_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "amatsukaze_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "tile_mul24_test.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no difference" in r.stdout
