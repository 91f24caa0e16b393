"""CPU side of the audio levels feature: the amts audio timeline (AMTSource::GetAudio restated in numpy, tests/audio_clips.py) against
AmtsFile.read_audio, the mute-section decision on hand-built records, chapter_exe's file with mute lines parsed the way
CMAnalyze::readSceneChanges parses it, and the new entry points in the header, the binding and the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import audio_clips as AC
from amtlib import ROOT

PROTOTYPES = (
    "int amtgpu_amts_audio_info(const AmtGpuAmtsFile* a, int* samples_per_frame, int64_t* num_samples);",
    "int amtgpu_amts_get_audio_frames(const AmtGpuAmtsFile* a, int* frameIndex, int64_t* waveOffset, int* waveLength);",
    "int amtgpu_amts_read_audio(const AmtGpuAmtsFile* a, const char* wavepath, int64_t start, int64_t count, int16_t* out);",
    "AmtGpuAudioLevels* amtgpu_audiolevels_create(AmtGpuContext* ctx, int sample_rate, int channels, int fps_num, int fps_den, "
    "int64_t num_samples);",
    "void amtgpu_audiolevels_destroy(AmtGpuAudioLevels* al);",
    "int64_t amtgpu_audiolevels_frame_start(const AmtGpuAudioLevels* al, int64_t frame);",
    "int amtgpu_audiolevels_batch(AmtGpuAudioLevels* al, const int16_t* d_pcm, int64_t pcm_first, int64_t pcm_count, int first_frame, "
    "int nframes, uint64_t* d_out);",
    "int amtgpu_audiolevels_amts(AmtGpuAudioLevels* al, const AmtGpuAmtsFile* a, const char* wavepath, int first_frame, int nframes, "
    "uint64_t* h_out);",
    "int amtgpu_cm_mute_sections(const uint64_t* levels, int nframes, int mute_level, int min_frames, int* start_out, int* end_out, "
    "int cap, int* nmute);",
    "int amtgpu_cm_write_chapter_exe_mute(const int* scene_changes, int nsc, const int* mute_start, const int* mute_end, int nmute, "
    "int nframes, int only_muted, const char* path);",
)
NAMES = tuple(re.search(r"(amtgpu_\w+)\(", p).group(1) for p in PROTOTYPES)


@pytest.fixture(scope="module")
def A():
    from amatsukaze_amd import build as b
    b.build()
    import amatsukaze_amd
    return amatsukaze_amd


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    return AC.AudioClip(tmp_path_factory.mktemp("audio"))


# ---- the audio timeline ----
def test_clip_has_the_shapes_the_reader_must_handle(clip):
    lengths = [f[2] for f in clip.frames]
    offs = [f[1] for f in clip.frames if f[2]]
    assert lengths[0] == 0 and lengths[1] == clip.spf * 4 and lengths.count(0) == 2 and 0 in lengths[2:-1]
    assert any(0 < n < clip.spf * 4 for n in lengths)                          # a waveLength GetAudio reads past
    assert offs != sorted(offs)                                                # not ascending in the file
    steps = [b - a for a, b in zip(offs, offs[1:])]
    assert clip.spf * 4 in steps and any(s != clip.spf * 4 for s in steps)     # contiguous runs and breaks
    assert any(o & 1 for o in offs)                                            # an odd file offset


def test_audio_info_is_the_reference_rule(A, clip, tmp_path):
    a = A.AmtsFile(clip.amtspath)
    assert a.audio_info() == (clip.spf, clip.spf * clip.naudio)
    fr = a.audio_frames()
    assert [tuple(int(v) for v in t) for t in zip(fr["frameIndex"], fr["waveOffset"], fr["waveLength"])] == clip.frames
    # no frame has a wave: 1024; no audio frames: 0, 0
    p = str(tmp_path / "z.dat")
    AC.write_amts(p, "s", "w", AC.VFMT, (2, 48000), [], [(0, 0, 0), (1, 0, 0), (2, 0, 0)])
    assert A.AmtsFile(p).audio_info() == (1024, 3072)
    AC.write_amts(p, "s", "w", AC.VFMT, (2, 48000), [], [])
    assert A.AmtsFile(p).audio_info() == (0, 0)


def read_cases(clip):
    spf, ns = clip.spf, clip.num_samples
    return [(0, ns), (0, 0), (5, 0), (spf // 2, 10), (spf - 1, 2), (spf + 7, 3 * spf + 11), (3 * spf, spf), (0, spf), (spf, 1),
            (ns - 5, 5), (ns - 5, 300), (ns, 17), (ns + 1000, 9), (6 * spf + 3, 3 * spf), (2 * spf - 1, ns)]


def test_read_audio_is_get_audio(A, clip):
    a = A.AmtsFile(clip.amtspath)
    whole = AC.get_audio_ref(clip.wave, clip.frames, 0, clip.num_samples)
    assert np.array_equal(whole, clip.timeline)                                # the restatement assembles what the clip was built from
    for start, count in read_cases(clip):
        want = AC.get_audio_ref(clip.wave, clip.frames, start, count)
        for wavepath in (None, clip.wavpath):                                  # the file's own audiopath, and an explicit one
            got = a.read_audio(start, count, wavepath)
            assert got.shape == (count, 2) and got.dtype == np.int16
            assert np.array_equal(got, want), (start, count)
    # past the end everything is zero; mid-frame starts and zero-length frames are in the list above
    assert not a.read_audio(clip.num_samples - 5, 300)[5:].any()
    z = clip.zero_frames[1]
    assert not a.read_audio(z * clip.spf, clip.spf).any() and a.read_audio(z * clip.spf - 1, clip.spf + 2)[[0, -1]].any()


def test_read_audio_refusals(A, clip, tmp_path):
    a = A.AmtsFile(clip.amtspath)
    for start, count in ((-1, 4), (0, -1)):
        with pytest.raises(A.AmtError):
            a.read_audio(start, count)
    with pytest.raises(A.AmtError):
        a.read_audio(0, 4, str(tmp_path / "absent.wav"))
    cut = str(tmp_path / "cut.wav")
    with open(cut, "wb") as f:
        f.write(clip.wave[:max(o for _, o, n in clip.frames if n) + 10])       # ends inside the frame that lies last in the file
    with pytest.raises(A.AmtError):
        a.read_audio(0, clip.num_samples, cut)
    p = str(tmp_path / "noaudio.dat")
    AC.write_amts(p, "s", clip.wavpath, AC.VFMT, (2, 48000), [], [])
    with pytest.raises(A.AmtError):
        A.AmtsFile(p).read_audio(0, 4)


# ---- mute sections ----
def records(peaks, counts=None):
    lv = np.zeros((len(peaks), 4), np.uint64)
    lv[:, 0] = peaks
    lv[:, 3] = 3200 if counts is None else counts
    return lv


def test_mute_sections_on_hand_built_records(A):
    L, M = 50, 10
    loud, quiet = L + 1, L
    # a run of min_frames - 1 (none), one of min_frames (one), runs touching frame 0 and the last frame
    peaks = [quiet] * M + [loud] + [quiet] * (M - 1) + [loud] * 2 + [0] * M + [loud] + [quiet] * (M + 3)
    lv = records(peaks)
    n = len(peaks)
    want = [(0, M - 1), (2 * M + 2, 3 * M + 1), (3 * M + 3, n - 1)]
    assert A.mute_sections(lv) == want == AC.mute_sections_ref(lv, L, M)
    assert A.mute_sections(lv, mute_level=L - 1) == [(2 * M + 2, 3 * M + 1)]      # PEAK == mute_level + 1 is not silent
    assert A.mute_sections(lv, min_frames=M - 1) == [(0, M - 1), (M + 1, 2 * M - 1)] + want[1:]
    assert A.mute_sections(lv, min_frames=M + 4) == []
    # frames that own no samples are silent whatever their other words say
    lv2 = records([loud] * 30, counts=[3200] * 8 + [0] * 12 + [3200] * 10)
    assert A.mute_sections(lv2) == [(8, 19)] == AC.mute_sections_ref(lv2, L, M)
    assert A.mute_sections(records([])) == []
    # cap smaller than the total: the total is reported, the first `cap` sections are written, the call returns 0
    from amatsukaze_amd import binding
    lib = binding.load()
    st, en, k = np.full(4, -7, np.int32), np.full(4, -7, np.int32), C.c_int()
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    assert lib.amtgpu_cm_mute_sections(p(lv), n, L, M, p(st), p(en), 2, C.byref(k)) == 0
    assert k.value == 3 and list(st) == [0, 2 * M + 2, -7, -7] and list(en) == [M - 1, 3 * M + 1, -7, -7]
    assert lib.amtgpu_cm_mute_sections(p(lv), n, L, M, p(st), p(en), 3, C.byref(k)) == 1 and k.value == 3
    assert lib.amtgpu_cm_mute_sections(p(lv), n, L, 0, p(st), p(en), 4, C.byref(k)) == 0          # min_frames below 1
    with pytest.raises(A.AmtError):
        A.mute_sections(lv, min_frames=0)


# ---- the file ----
RE0 = re.compile(r"mute\s*(\d+):\s*(\d+)\s*-\s*(\d+).*")          # CMAnalyze.hpp:426-427
RE1 = re.compile(r"\s*SCPos:\s*(\d+).*")


def parse_chapter_exe(path):
    """CMAnalyze::readSceneChanges (CMAnalyze.hpp:411-439): lines up to one that starts with "----" are header; then re0 is tried
    first, re1 second.  Returns the events in file order: ("mute", k, a, b) / ("sc", frame)"""
    lines = open(path).read().split("\n")
    body = None
    for i, line in enumerate(lines):
        if line.startswith("----"):
            body = lines[i + 1:]
            break
    assert body is not None
    events = []
    for line in body:
        m = RE0.search(line)
        if m:
            events.append(("mute", int(m.group(1)), int(m.group(2)), int(m.group(3))))
            continue
        m = RE1.search(line)
        if m:
            events.append(("sc", int(m.group(1))))
    return events


SECTIONS = [(0, 11), (40, 49), (100, 160), (161, 175), (290, 299)]
NFRAMES = 300
#            in s0  s0's end+1  none  s1 start  end+1  end+2  before s2  s2 == s3 start - ...                     last frame
SCENE_CHANGES = [0, 5, 12, 13, 30, 40, 50, 51, 99, 100, 130, 161, 176, 177, 250, 299]
MEMBERS = [0, 5, 12, 40, 50, 100, 130, 161, 176, 299]


def test_chapter_exe_file_with_mute_lines(A, tmp_path):
    path = str(tmp_path / "chapter_exe.txt")
    A.write_chapter_exe(path, SCENE_CHANGES, NFRAMES, mute=SECTIONS)
    ev = parse_chapter_exe(path)
    sc = [e[1] for e in ev if e[0] == "sc"]
    assert sc == SCENE_CHANGES and sc == sorted(sc)                            # what the reference's reader collects: unchanged, ascending
    assert [e[1:] for e in ev if e[0] == "mute"] == [(k + 1, a, b) for k, (a, b) in enumerate(SECTIONS)]
    # every section's line precedes its members -- and every scene change at or behind its start
    for a, b in SECTIONS:
        at = ev.index(next(e for e in ev if e[0] == "mute" and e[2] == a))
        assert all(ev.index(("sc", s)) > at for s in SCENE_CHANGES if s >= a)
        assert all(ev.index(("sc", s)) < at for s in SCENE_CHANGES if s < a)
    # the same scene-change list as the file without mute lines gives, and that writer's line format
    plain = str(tmp_path / "plain.txt")
    A.write_chapter_exe(plain, SCENE_CHANGES, NFRAMES)
    assert [e[1] for e in parse_chapter_exe(plain)] == sc
    sc_lines = lambda p: [l for l in open(p).read().split("\n") if "SCPos" in l]
    assert sc_lines(plain) == sc_lines(path)
    text = open(path).read()
    assert "\nmute 1: 0 - 11\n" in text and "\nmute 5: 290 - 299\n" in text and text.endswith("\n")

    A.write_chapter_exe(path, SCENE_CHANGES, NFRAMES, mute=SECTIONS, only_muted=True)
    ev = parse_chapter_exe(path)
    assert [e[1] for e in ev if e[0] == "sc"] == MEMBERS                       # end + 1 stays (12, 50, 176), end + 2 goes (13, 51, 177)
    assert [e[1:] for e in ev if e[0] == "mute"] == [(k + 1, a, b) for k, (a, b) in enumerate(SECTIONS)]
    # no scene changes, no sections
    A.write_chapter_exe(path, [], NFRAMES, mute=SECTIONS)
    assert [e[0] for e in parse_chapter_exe(path)] == ["mute"] * len(SECTIONS)
    A.write_chapter_exe(path, SCENE_CHANGES, NFRAMES, mute=[], only_muted=True)
    assert parse_chapter_exe(path) == []
    A.write_chapter_exe(path, SCENE_CHANGES, NFRAMES, mute=[])
    assert [e[1] for e in parse_chapter_exe(path)] == SCENE_CHANGES


@pytest.mark.parametrize("sc,mute", [
    ([5, 4], SECTIONS),                                     # scene changes not ascending
    ([1], [(40, 49), (0, 11)]),                             # sections not ascending
    ([1], [(0, 11), (11, 20)]),                             # overlapping
    ([1], [(12, 11)]),                                      # start > end
    ([1], [(-1, 5)]),                                       # outside the clip ...
    ([1], [(290, 300)]),                                    # ... at either end
], ids=["sc-unsorted", "sections-unsorted", "overlap", "start-after-end", "negative-start", "end-at-nframes"])
def test_chapter_exe_refusals(A, tmp_path, sc, mute):
    with pytest.raises(A.AmtError):
        A.write_chapter_exe(str(tmp_path / "refused.txt"), sc, NFRAMES, mute=mute)


def test_chapter_exe_unwritable_path(A, tmp_path):
    with pytest.raises(A.AmtError):
        A.write_chapter_exe(str(tmp_path / "no_such_dir" / "x.txt"), [1], NFRAMES, mute=[(0, 11)])


# ---- header, binding, library ----
def squeeze(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_binding_and_library_carry_the_entry_points(A):
    raw = open(os.path.join(ROOT, "include", "amt_gpu.h")).read()
    hdr = squeeze(raw)
    for proto in PROTOTYPES:
        assert squeeze(proto) in hdr, proto
    assert re.search(r"^#define AMTGPU_ABI_VERSION 5\b", raw, re.M)            # additions only
    for name, value in (("WORDS", 4), ("PEAK", 0), ("SUMABS", 1), ("SUMSQ", 2), ("COUNT", 3)):
        assert re.search(rf"^#define AMTGPU_AL_{name}\s+{value}\b", raw, re.M), name
    assert "no \"mute\" lines (audio is out of scope)" not in raw
    from amatsukaze_amd import binding, build as b
    c_i, c_p, c_s, c_i64 = C.c_int, C.c_void_p, C.c_char_p, C.c_int64
    want = {
        "amtgpu_amts_audio_info": (c_i, [c_p, c_p, c_p]),
        "amtgpu_amts_get_audio_frames": (c_i, [c_p, c_p, c_p, c_p]),
        "amtgpu_amts_read_audio": (c_i, [c_p, c_s, c_i64, c_i64, c_p]),
        "amtgpu_audiolevels_create": (c_p, [c_p, c_i, c_i, c_i, c_i, c_i64]),
        "amtgpu_audiolevels_destroy": (None, [c_p]),
        "amtgpu_audiolevels_frame_start": (c_i64, [c_p, c_i64]),
        "amtgpu_audiolevels_batch": (c_i, [c_p, c_p, c_i64, c_i64, c_i, c_i, c_p]),
        "amtgpu_audiolevels_amts": (c_i, [c_p, c_p, c_s, c_i, c_i, c_p]),
        "amtgpu_cm_mute_sections": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_i, c_p]),
        "amtgpu_cm_write_chapter_exe_mute": (c_i, [c_p, c_i, c_p, c_p, c_i, c_i, c_i, c_s]),
    }
    assert set(want) == set(NAMES)
    for name, sig in want.items():
        assert binding.SIGNATURES[name] == sig, name
    assert {"audio_kernels.hip", "amt_gpu_audio.hip"} <= set(b.SOURCES)
    out = subprocess.run(["nm", "-D", "--defined-only", b.OUT], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(\S+)$", out, re.M))
    assert set(NAMES) <= exported
    assert binding.load().amtgpu_abi_version() == 5
    for name in ("AudioLevels", "mute_sections", "write_chapter_exe"):
        assert name in A.__all__ and hasattr(A, name)


def test_stand_alone_reader_program(tmp_path):
    """tests/cpp/amts_audio_host_test.cpp: the reader driven from C++ into exact-size heap buffers (the program a host sanitizer build
    runs; its header has the command).  Built here as an ordinary program from amts_file.cpp alone: ROCm's headers, none of its runtime"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "amts_audio_host_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "amatsukaze_amd", "csrc", "amts_file.cpp"),
                           os.path.join(ROOT, "tests", "cpp", "amts_audio_host_test.cpp"), "-o", exe])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
