"""The source/destination rule of the resident post-process chain (tests/cpp/plane_pair_test.cpp over amatsukaze_amd/csrc/plane_pair.hpp).

amtgpu_kfm_render*, amtgpu_resize_run*, amtgpu_temporal_nr* and amtgpu_deband_run take a source and a destination AmtGpuSurfaces and must
establish the same facts before a kernel writes HBM through them: layout, the object's bits, non-negative strides, rows that fit their
pitch, a pair in kind, byte pitches that fit an int, destination frames that do not overlap each other, and no destination plane whose
byte range touches a source plane's.  That text is one HIP-free header, and the program checks it without a GPU:

  span rule      planes_touch against a byte map -- every byte of [first byte of frame 0, last byte of frame n - 1] of each source plane
                 marked, a placement refused exactly when a destination plane's range holds a marked byte -- on every combination of:
                 luma 4x4 and 6x4 containers, source and destination each; es 1 and 2; pitch the row and the row + 3 containers; stride
                 tight and tight + 5 containers; 1..3 source and 1..2 destination frames; planar and interleaved; each destination plane
                 in turn at every container offset of an arena one destination frame larger than the source on either side.  Interleaved
                 sides also with garbage for a third plane (a pointer into the other side, a pointer that is no address), in the batch
                 and planted behind it: it changes nothing.  A plane that starts on the source's last byte (refused), one byte behind it
                 (accepted) and an interleaved UV plane inside the source's luma (refused) must have occurred, and both answers.
  frame overlap  frames_overlap against a map of frame 0, for every stride from 0 to tight + 5 containers, luma and chroma; one frame
                 alone is never refused; a stride of exactly (rows - 1) * pitch + row bytes passes and one container less does not.
  messages       every shared refusal of the four entry points equals, byte for byte, the literal that stood in that entry point's file,
                 in the order layout, bits, stride, pitch; planar-only against every layout, an object's bits against none.
  2 GiB          a 16-bit side with a pitch of 2^30 + 16 containers is refused by all four before anything is formed from the pitch;
                 2^30 containers of 8 bits and 2^30 - 1 of 16 bits are not.

The program exits non-zero at the first difference and prints the inputs."""
import os
import re
import subprocess

import amtlib

ROOT = amtlib.ROOT
CSRC = os.path.join(ROOT, "amatsukaze_amd", "csrc")
CHAIN = {"amt_gpu_render.hip": "kRenderPair", "amt_gpu_resize.hip": "kResizePair", "amt_gpu_tnr.hip": "kTemporalNRPair", "amt_gpu_deband.hip": "kDebandPair"}


def test_the_rule_against_a_byte_map_and_the_entry_points_words(tmp_path):
    out = str(tmp_path / "plane_pair_test")
    # no ROCm include path: the header and what it includes hold no HIP
    c = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "plane_pair_test.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert c.returncode == 0 and not c.stderr.strip(), c.stderr
    r = subprocess.run([out], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no difference" in r.stdout
    accepted, refused = (int(v) for v in re.search(r"span rule: (\d+) placements accepted, (\d+) refused", r.stdout).groups())
    assert accepted > 100000 and refused > 100000


def test_the_rule_stands_in_one_file():
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f))}
    for text in ("struct Span", "plane_span", "destination frames overlap each other", "pitch above 2 GiB", "planar, LSB-aligned planes only (",
                 "converts no layouts", "was created for", "byte range overlaps the source's"):
        assert [f for f, t in files.items() if text in t] == ["plane_pair.hpp"], text
    # ([AMTSource]'s and [LogoFind]'s own messages with the same words are not part of the rule)
    assert [f for f, t in files.items() if "pitch smaller than the row" in t] == ["amt_gpu_ingest.hip", "plane_pair.hpp"]
    assert '"[AMTSource] pitch smaller than the row"' in files["amt_gpu_ingest.hip"]
    assert [f for f, t in files.items() if "negative frame stride" in t] == ["amt_gpu_logofind.hip", "plane_pair.hpp"]
    assert '"[LogoFind] pitch below the width or negative frame stride"' in files["amt_gpu_logofind.hip"]
    for f, rule in CHAIN.items():
        assert re.search(rf"^const PlanePairRule& kPair = {rule};$", files[f], re.M), f
        assert all(f"kPair.{call}(" in files[f] for call in ("side", "bytes", "disjoint")) and not re.search(r"\bRowsAt\s*\{", files[f]), f
        assert ("kPair.in_kind(" in files[f]) == (f != "amt_gpu_deband.hip"), f            # deband takes one layout
    assert [f for f, t in files.items() if "PlanePairRule" in t] == sorted(CHAIN) + ["plane_pair.hpp"]
    # the header and the FrameBatch it takes hold no HIP; kernels.hpp takes FrameBatch from there
    for f in ("plane_pair.hpp", "frame_batch.h"):
        assert not re.search(r"hip/|__global__|__device__|hipError_t|hipStream_t", files[f]), f
    assert [f for f, t in files.items() if re.search(r"\bstruct\s+FrameBatch\s*\{", t)] == ["frame_batch.h"]
    assert re.search(r'^#include "frame_batch\.h"', files["kernels.hpp"], re.M) and "plane_batch_from" not in files["kernels.hpp"].replace("plane_batch_from: frame_batch.h", "")
