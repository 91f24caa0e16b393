"""The one lane-width rule of the copy-shaped launchers (tests/cpp/lane_rule_test.cpp over amatsukaze_amd/csrc/lane_rule.h).

How many bytes a lane may move is decided from the alignment of every address, frame stride, row pitch and row length of an access; it is
all that stands between a caller's odd offset and a misaligned vector access.  Six launch sites used to write that decision out by hand
(the weave's, in amt_gpu_ingest.hip, still does and is not compared here).
The program carries those six expressions as they stood and compares each with the function of lane_rule.h that replaced it, on every
combination of this domain (addresses are a page-aligned base plus the offset; es is 1 and 2 everywhere):

  P32 = offsets 0..31; P5 = {0, 1, 2, 4, 8}; S14 = {0, 1, 2, 4, 6, 8, 12, 16, 24, 32, 48, 1472, 1474, 2944}; S6 = {0, 1, 2, 4, 8, 1474};
  W64 = 1..64 samples; W14 = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 33, 48, 63, 64}; W8 = {1, 2, 3, 4, 8, 16, 17, 64}

  scan keep, luma           src P32, store P32, stride S14 (samples), pitch S14, w W64
  scan keep, chroma         srcU P32, srcV / storeU / storeV P5, stride S6, pitch S6, wUV W14
  surfaces extract, luma    src P32, dst P5, source and destination stride and pitch S6 each, w W14
  surfaces extract, chroma  srcU P32, srcV / dstU / dstV P5, the four strides and pitches S6 each, wUV W8; planar, and interleaved with
                            its 16 / 8 and 4 / 2 byte halves and pairC
  surface Delogo, luma      src P32, dst P32, stride S14 (bytes), pitch S14 (containers), w W64
  surface Delogo, chroma    sU P32, sV / U / V P5, stride S6, pitch S6, wUV W64; planar and interleaved
  Delogo pair, luma         src P32, dst P32, stride S14 (samples: the byte strides the ABI layer lets through), pitch S14, imgx 0..7, w W14
  Delogo pair, chroma       srcU P32, srcV / dstU / dstV P5, stride S6 (samples), pitch S6, cx 0..3, wUV W14
  ingest rows               src P32, dst P32, both strides S14, chunk 1..64 bytes
  render vec                srcY P32, the other five planes {0, 8}, the four strides and the four pitches {0, 8, -16}

The program exits non-zero at the first difference and prints the site and the inputs."""
import os
import subprocess

import amtlib

ROOT = amtlib.ROOT


def test_every_site_selects_what_it_selected(tmp_path):
    out = str(tmp_path / "lane_rule_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "amatsukaze_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "lane_rule_test.cpp"), "-o", out])
    r = subprocess.run([out], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no difference" in r.stdout
