"""Inputs and numpy references of the audio tests (tests/test_audio_host.py, tests/test_gpu_audio_levels.py, tests/test_gpu_audio_spans.py):
an amts file with its wave file, AMTSource::GetAudio restated in numpy, the per-video-frame level records and the mute sections restated
in numpy, and the kernel's split of a span restated in Python (for the checks that a case list reaches what it says)."""
import os

import numpy as np

from amts_util import write_amts

VFMT = (0, 1440, 1080, 1440, 1080, 4, 3, 30000, 1001, 1, 1, 1, False, True)


class AudioClip:
    """An amts file whose FilterAudioFrame list has: a first frame with waveLength 0 (samples-per-frame comes from the second), one more
    zero-length frame in the middle, one frame whose waveLength is 8 bytes short of what GetAudio reads for it, and wave offsets that are
    neither ascending nor contiguous: the frames lie in the wave file in runs of 1..5, the second half of the runs in front of the first,
    with gaps of junk between the runs (odd offsets included).
    timeline: the (naudio * spf, 2) int16 audio GetAudio assembles (zeros where a frame has no wave)."""

    def __init__(self, dirpath, naudio=12, spf=256, seed=7, samples=None, sample_rate=48000, name="clip"):
        rng = np.random.default_rng(seed)
        self.naudio, self.spf, self.sample_rate = naudio, spf, sample_rate
        self.zero_frames = (0, naudio // 2 + 1)
        self.short_frame = 3
        want = (rng.integers(-32768, 32768, (naudio * spf, 2)).astype(np.int16) if samples is None
                else np.ascontiguousarray(samples, np.int16).reshape(naudio * spf, 2).copy())
        for z in self.zero_frames:
            want[z * spf:(z + 1) * spf] = 0
        self.timeline = want
        # runs of frames that are contiguous in the file
        runs, k = [], 0
        while k < naudio:
            n = int(rng.integers(1, 6))
            runs.append(list(range(k, min(naudio, k + n))))
            k += n
        order = runs[len(runs) // 2:] + runs[:len(runs) // 2]
        blob = bytearray(rng.integers(0, 256, 44, dtype=np.uint8).tobytes())          # where a RIFF header would be
        offsets = {}
        for run in order:
            blob += rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()      # junk between the runs
            for f in run:
                if f in self.zero_frames:
                    continue                                                  # nothing in the file (what follows stays contiguous)
                offsets[f] = len(blob)
                blob += want[f * spf:(f + 1) * spf].tobytes()
        blob += rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        self.wave = bytes(blob)
        self.frames = []
        for f in range(naudio):
            if f in self.zero_frames:
                self.frames.append((f, 12345 + f, 0))                         # an offset that must never be looked at
            else:
                self.frames.append((f, offsets[f], spf * 4 - (8 if f == self.short_frame else 0)))
        self.wavpath = os.path.join(str(dirpath), name + ".wav")
        self.amtspath = os.path.join(str(dirpath), name + ".dat")
        with open(self.wavpath, "wb") as fh:
            fh.write(self.wave)
        write_amts(self.amtspath, "C:\\ts\\src.ts", self.wavpath, VFMT, (2, sample_rate), [], self.frames)

    @property
    def num_samples(self):
        return self.naudio * self.spf


def get_audio_ref(wave: bytes, frames, start, count):
    """AMTSource::MakeVideoInfo's samples-per-frame rule and AMTSource::GetAudio (AMTSource.hpp:239-247, 782-817), statement by statement,
    for a 16-bit stereo wave: (count, 2) int16"""
    spf = 1024
    for _, _, length in frames:
        if length != 0:
            spf = length // 4
            break
    out = bytearray(count * 4)
    pos = 0
    idx, off = start // spf, start % spf
    while count > 0 and idx < len(frames):
        nbytes = min(spf * 4 - off * 4, count * 4)
        _, woff, wlen = frames[idx]
        if wlen != 0:
            piece = wave[woff + off * 4:woff + off * 4 + nbytes]
            assert len(piece) == nbytes, "the test's own wave file is too short"
            out[pos:pos + nbytes] = piece
        pos += nbytes
        count -= nbytes // 4
        idx, off = idx + 1, 0
    return np.frombuffer(bytes(out), np.int16).reshape(-1, 2)


def frame_start(n, sample_rate, fps_num, fps_den):
    return n * sample_rate * fps_den // fps_num


def levels_ref(pcm, sample_rate, channels, fps_num, fps_den, num_samples, first_frame, nframes):
    """(nframes, 4) uint64 {PEAK, SUMABS, SUMSQ, COUNT}; pcm: the timeline from sample-frame 0 on, (>= num_samples, channels) int16"""
    pcm = np.asarray(pcm).reshape(-1, channels)
    out = np.zeros((nframes, 4), np.uint64)
    for i in range(nframes):
        s0 = min(frame_start(first_frame + i, sample_rate, fps_num, fps_den), num_samples)
        s1 = min(frame_start(first_frame + i + 1, sample_rate, fps_num, fps_den), num_samples)
        x = np.abs(pcm[s0:s1].astype(np.int64)).reshape(-1)
        if x.size:
            out[i] = (int(x.max()), int(x.sum()), int((x * x).sum()), x.size)
    return out


def levels_ref_window(pcm, pcm_first, sample_rate, channels, fps_num, fps_den, num_samples, first_frame, nframes):
    """levels_ref for a window of the timeline: pcm's row 0 is sample-frame pcm_first, (>= the frames' cover, channels) int16.  Positions
    are Python integers throughout, so a batch may lie anywhere in the timeline; a span outside the window is an error, not a guess"""
    pcm = np.asarray(pcm).reshape(-1, channels)
    out = np.zeros((nframes, 4), np.uint64)
    for i in range(nframes):
        s0 = min(frame_start(int(first_frame) + i, sample_rate, fps_num, fps_den), int(num_samples))
        s1 = min(frame_start(int(first_frame) + i + 1, sample_rate, fps_num, fps_den), int(num_samples))
        if s1 <= s0:
            continue
        assert int(pcm_first) <= s0 and s1 - int(pcm_first) <= pcm.shape[0], "the window does not cover the frame's span"
        x = [abs(int(v)) for v in pcm[s0 - int(pcm_first):s1 - int(pcm_first)].reshape(-1)]
        out[i] = (max(x), sum(x), sum(v * v for v in x), len(x))
    return out


class SpanSplit:
    """audio_levels_kernel's split of the elements [e0, e1) of a buffer whose address has the low four bits `mis` (audio_span.h,
    restated): byte offsets a0 <= b0 <= b1 <= a1, head and tail in elements, body in 16-byte chunks and in groups of 512 chunks"""

    def __init__(self, mis, e0, e1):
        assert mis % 2 == 0 and 0 <= mis < 16 and e1 > e0
        self.a0, self.a1 = 2 * e0, 2 * e1
        self.b0 = min(((self.a0 + mis + 15) & ~15) - mis, self.a1)
        self.b1 = max(((self.a1 + mis) & ~15) - mis, self.b0)
        self.nhead, self.ntail = (self.b0 - self.a0) // 2, (self.a1 - self.b1) // 2
        self.nchunks = (self.b1 - self.b0) // 16
        self.groups = -(-self.nchunks // 512)
        self.whole_head = self.nchunks == 0 and self.ntail == 0           # the span holds no 16-byte boundary behind its start


def span_split(mis, e0, e1):
    return SpanSplit(mis, e0, e1)


def mute_sections_ref(levels, mute_level, min_frames):
    silent = [int(r[3]) == 0 or int(r[0]) <= mute_level for r in levels]
    out, run = [], 0
    for n, s in enumerate(silent + [False]):
        if s:
            run += 1
            continue
        if run >= min_frames:
            out.append((n - run, n - 1))
        run = 0
    return out


# ---- the end-to-end clip: 48 kHz stereo under 30000/1001 video, three silences of 9, 10 and 40 video frames at peak 50 between noise at
# peak 51.  Only the runs of at least 10 frames are mute sections.
E2E_RATE, E2E_FPS = 48000, (30000, 1001)
E2E_LAYOUT = ((3, False), (9, True), (2, False), (10, True), (3, False), (40, True), (3, False))      # (video frames, silent)
E2E_SECTIONS = [(14, 23), (27, 66)]


def e2e_clip(dirpath):
    spf = 1024
    b = lambda n: frame_start(n, E2E_RATE, *E2E_FPS)
    nvideo = sum(n for n, _ in E2E_LAYOUT)
    naudio = -(-b(nvideo) // spf)                     # the timeline ends inside video frame `nvideo`, which is noise
    rng = np.random.default_rng(11)
    s = rng.integers(-51, 52, (naudio * spf, 2)).astype(np.int16)
    f = 0
    for n, silent in E2E_LAYOUT:
        if silent:
            s[b(f):b(f + n)] = rng.integers(-50, 51, (b(f + n) - b(f), 2)).astype(np.int16)
        f += n
    clip = AudioClip(dirpath, naudio=naudio, spf=spf, seed=5, samples=s, sample_rate=E2E_RATE, name="e2e")
    # every video frame reaches exactly its planned peak (the zero-length audio frames included: they are shorter than a video frame)
    nframes = nvideo + 1
    lv = levels_ref(clip.timeline, E2E_RATE, 2, *E2E_FPS, clip.num_samples, 0, nframes)
    plan = sum(([50 if silent else 51] * n for n, silent in E2E_LAYOUT), []) + [51]
    assert [int(v) for v in lv[:, 0]] == plan and int(lv[-1, 3]) > 0
    assert frame_start(nframes, E2E_RATE, *E2E_FPS) >= clip.num_samples
    return clip, nframes
