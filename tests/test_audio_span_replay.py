"""The audio level kernel's span arithmetic replayed on the host (tests/cpp/audio_span_replay.cpp over amatsukaze_amd/csrc/audio_span.h).

audio_levels_kernel cuts a video frame's PCM span into a head of up to 7 elements, a body of aligned 16-byte chunks read in groups of
512 (lanes without a chunk re-read the last one) and a tail of up to 7 elements; that arithmetic is all that keeps a load inside the
span.  The kernel calls the functions of audio_span.h for it, and the program calls the same functions for every lane of every load of

  every even pointer misalignment 0..14  x  every span start 0..15 elements  x  every length 0..8300 elements (0 to 1025 chunks and a
  little more), and lengths of 24 and 25 groups (the emptiest and the full last group of each, and a last group of one chunk)

and exits non-zero with the offending tuple unless head, body and tail partition the span, the body is aligned, every byte of every
load (clamped re-reads and the idle lanes' dropped element included) lies inside the span, every chunk and every head / tail element
is taken exactly once, and an empty span issues no load."""
import os
import subprocess

import amtlib

ROOT = amtlib.ROOT


def test_every_load_stays_inside_its_span_and_every_element_counts_once(tmp_path):
    out = str(tmp_path / "audio_span_replay")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "amatsukaze_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "audio_span_replay.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every rule holds" in r.stdout
