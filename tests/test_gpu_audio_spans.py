"""The audio level kernel at every way its span arithmetic can fall (amatsukaze_amd/csrc/audio_span.h; replayed load by load on the host
in tests/test_audio_span_replay.py): spans of zero chunks with every head and tail size, spans the head takes whole, empty spans inside
the timeline, bodies that end on and next to a group boundary (511, 512, 513, 1024, 1025 chunks), last groups of one chunk and of one
wave, 4 and 24 groups, every channel count, and a batch two billion frames into the timeline.

Every comparison is np.array_equal on the four uint64 words of every record against numpy (audio_clips.levels_ref; the far batch against
audio_clips.levels_ref_window, which takes the PCM of the batch alone).  Every device buffer holds 32767 in front of and behind the PCM
handed over, and every noise sample inside the timeline is below 32767 (`// 2`): a load outside a span shows in PEAK.  The tests without
the gpu mark check on the CPU, with audio_clips.span_split, that the case lists reach what they say."""
import numpy as np
import pytest

import audio_clips as AC

gpu = pytest.mark.gpu

FRONT, BACK = 8, 24          # elements of 32767 around the PCM handed over; FRONT * 2 bytes keeps the tensor's alignment
SENTINEL = 32767


@pytest.fixture(scope="module")
def A():
    import amatsukaze_amd
    return amatsukaze_amd


@pytest.fixture(scope="module")
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


class Timeline:
    """the five numbers of the span rule, and b(n)"""

    def __init__(self, rate, channels, fps, num_samples):
        self.rate, self.channels, self.fps, self.num_samples = rate, channels, fps, num_samples

    def b(self, n):
        return min(AC.frame_start(n, self.rate, *self.fps), self.num_samples)

    def make(self, A, ctx):
        return A.AudioLevels(ctx, self.rate, self.channels, *self.fps, self.num_samples)

    def splits(self, base_off, first_frame, nframes, pcm_first=None):
        """the kernel's split of every frame of a batch whose buffer starts base_off elements behind a 16-byte boundary and at
        sample-frame pcm_first (default: the batch's own cover); None for an empty span"""
        pcm_first = self.b(first_frame) if pcm_first is None else pcm_first
        out = []
        for n in range(first_frame, first_frame + nframes):
            e0, e1 = (self.b(n) - pcm_first) * self.channels, (self.b(n + 1) - pcm_first) * self.channels
            out.append(AC.span_split(2 * base_off % 16, e0, e1) if e1 > e0 else None)
        return out


def noise(seed, samples, channels):
    """below 32767 (and above -32767) everywhere"""
    return (np.random.default_rng(seed).integers(-32768, 32768, (samples, channels)) // 2).astype(np.int16)


def run_cover(ctx, al, tl, window, win_first, first_frame, nframes, base_off):
    """records of [first_frame, first_frame + nframes) from a device buffer that holds exactly the frames' cover, base_off elements
    behind a 16-byte boundary, between sentinels.  window: (n, channels) int16 whose row 0 is sample-frame win_first"""
    import torch
    lo, hi = tl.b(first_frame), tl.b(first_frame + nframes)
    payload = np.asarray(window).reshape(-1, tl.channels)[lo - win_first:hi - win_first].reshape(-1)
    assert payload.size == (hi - lo) * tl.channels
    host = np.full(FRONT + base_off + payload.size + BACK, SENTINEL, np.int16)
    host[FRONT + base_off:FRONT + base_off + payload.size] = payload
    flat = torch.from_numpy(host).cuda()
    assert flat.data_ptr() % 16 == 0
    out = al.run_device(flat[FRONT + base_off:FRONT + base_off + payload.size], lo, first_frame, nframes)
    ctx.synchronize()
    return out.cpu().numpy().astype(np.uint64)


def want_of(tl, timeline, first_frame, nframes):
    return AC.levels_ref(timeline, tl.rate, tl.channels, *tl.fps, tl.num_samples, first_frame, nframes)


# ---- a. chunk-count sweep: mono, sample_rate = L, 1 fps: every span is exactly L elements, b(n) = n * L -------------------------------
SWEEP_C = (0, 1, 62, 63, 64, 65, 510, 511, 512, 513, 1023, 1024, 1025)
SWEEP_L = tuple(8 * c + d for c in SWEEP_C for d in (1, 7))
SWEEP_FRAMES = 16
SWEEP_BASES = (0, 1)          # the buffer's base 16-byte aligned, and one element in


def sweep_timeline(L):
    return Timeline(L, 1, (1, 1), SWEEP_FRAMES * L)


def test_case_list_is_what_it_says():
    splits = [s for L in SWEEP_L for base in SWEEP_BASES for s in sweep_timeline(L).splits(base, 0, SWEEP_FRAMES)]
    assert all(s is not None for s in splits)
    assert {0, 1, 63, 64, 65, 511, 512, 513, 1024, 1025} <= {s.nchunks for s in splits}
    assert {s.nhead for s in splits} == set(range(8)) and {s.ntail for s in splits} == set(range(8))
    assert {s.nhead for s in splits if s.nchunks == 0} == set(range(8))          # zero-chunk spans with every head ...
    assert {s.ntail for s in splits if s.nchunks == 0} == set(range(8))          # ... and every tail size
    assert any(s.whole_head for s in splits)
    # a last group of exactly one chunk, of one wave less / exactly / more than one wave, and a full one
    assert {1, 63, 64, 65, 0} <= {s.nchunks % 512 for s in splits if s.nchunks}
    assert {1, 2, 3} <= {s.groups for s in splits}
    # every case walks the start of its spans through all eight even byte offsets
    for L in SWEEP_L:
        for base in SWEEP_BASES:
            assert {(2 * base + 2 * n * L) % 16 for n in range(SWEEP_FRAMES)} == set(range(0, 16, 2)), (L, base)
    assert max(SWEEP_L) * SWEEP_FRAMES == 16 * 8207


@gpu
@pytest.mark.parametrize("base", SWEEP_BASES)
def test_chunk_count_sweep(A, ctx, base):
    for L in SWEEP_L:
        tl = sweep_timeline(L)
        pcm = noise(100 + L, tl.num_samples, 1)
        got = run_cover(ctx, tl.make(A, ctx), tl, pcm, 0, 0, SWEEP_FRAMES, base)
        want = want_of(tl, pcm, 0, SWEEP_FRAMES)
        assert np.array_equal(got, want), (L, base, np.argwhere(got != want)[:4].tolist())
        assert np.all(got[:, 3] == L) and got[:, 0].max() < SENTINEL


# ---- b. many groups and extremes ------------------------------------------------------------------------------------------------------
MANY = Timeline(48000, 2, (1, 1), 4 * 48000 + 1001)          # 4 frames of 12 000 chunks, a fifth cut short by num_samples
HIRES = Timeline(192000, 2, (24000, 1001), 5 * 8008)          # 5 frames of 2002 chunks


def test_many_groups_case_list():
    full = MANY.splits(0, 0, 5)
    assert [s.nchunks for s in full[:4]] == [12000] * 4 and [s.groups for s in full[:4]] == [24] * 4
    assert MANY.b(5) - MANY.b(4) == 1001 and AC.frame_start(5, 48000, 1, 1) > MANY.num_samples
    assert {s.groups for s in MANY.splits(1, 0, 5)[:4]} == {24}
    assert [s.nchunks for s in HIRES.splits(0, 0, 5)] == [2002] * 5 and {s.groups for s in HIRES.splits(0, 0, 5)} == {4}
    assert (MANY.num_samples * 2 + FRONT + BACK + 1) * 2 < 1 << 20          # the largest upload of this file


@gpu
@pytest.mark.parametrize("base", (0, 1))
def test_24_groups_noise(A, ctx, base):
    pcm = noise(21, MANY.num_samples, 2)
    got = run_cover(ctx, MANY.make(A, ctx), MANY, pcm, 0, 0, 5, base)
    assert np.array_equal(got, want_of(MANY, pcm, 0, 5))
    assert [int(c) for c in got[:, 3]] == [96000] * 4 + [2002] and got[:, 0].max() < SENTINEL


@gpu
@pytest.mark.parametrize("base", (0, 1))
def test_24_groups_all_minus_32768(A, ctx, base):
    pcm = np.full((MANY.num_samples, 2), -32768, np.int16)
    got = run_cover(ctx, MANY.make(A, ctx), MANY, pcm, 0, 0, 5, base)
    count = np.array([96000] * 4 + [2002], np.uint64)
    closed = np.stack([np.full(5, 32768, np.uint64), count << np.uint64(15), count << np.uint64(30), count], axis=1)
    assert np.array_equal(got, closed)
    assert np.array_equal(closed, want_of(MANY, pcm, 0, 5))


@gpu
@pytest.mark.parametrize("base", (0, 1))
def test_4_groups_192k(A, ctx, base):
    pcm = noise(22, HIRES.num_samples, 2)
    got = run_cover(ctx, HIRES.make(A, ctx), HIRES, pcm, 0, 0, 5, base)
    assert np.array_equal(got, want_of(HIRES, pcm, 0, 5))
    assert np.all(got[:, 3] == 16016) and got[:, 0].max() < SENTINEL


# ---- c. tiny and empty spans ----------------------------------------------------------------------------------------------------------
TINY_PAIRS = ((100, (120, 1)), (7, (2, 1)))          # span lengths 0 and 1; 3 and 4 sample-frames
TINY_CHANNELS = (1, 3, 8)
TINY_FRAMES = 24
TINY_BASES = tuple(range(8))


def tiny_timeline(rate, fps, channels):
    return Timeline(rate, channels, fps, AC.frame_start(TINY_FRAMES, rate, *fps))


def test_tiny_case_list():
    fast = tiny_timeline(100, (120, 1), 1)
    lengths = [fast.b(n + 1) - fast.b(n) for n in range(TINY_FRAMES)]
    assert set(lengths) == {0, 1}
    # empty spans IN FRONT OF num_samples: fps exceeds the sample rate, nothing is cut
    assert [n for n in range(TINY_FRAMES) if lengths[n] == 0 and fast.b(n) < fast.num_samples]
    slow = tiny_timeline(7, (2, 1), 1)
    assert {slow.b(n + 1) - slow.b(n) for n in range(TINY_FRAMES)} == {3, 4}
    # 8 channels, one sample-frame: 16 bytes that are one aligned chunk, or a head and a tail around a boundary
    eight = [s for base in TINY_BASES for s in tiny_timeline(100, (120, 1), 8).splits(base, 0, TINY_FRAMES) if s is not None]
    assert any((s.nhead, s.nchunks, s.ntail) == (0, 1, 0) for s in eight)
    assert any(s.nchunks == 0 and s.nhead > 0 and s.ntail > 0 and s.nhead + s.ntail == 8 for s in eight)
    every = [s for rate, fps in TINY_PAIRS for ch in TINY_CHANNELS for base in TINY_BASES
             for s in tiny_timeline(rate, fps, ch).splits(base, 0, TINY_FRAMES) if s is not None]
    assert any(s.whole_head for s in every) and {s.nchunks for s in every} == {0, 1, 2, 3, 4}


@gpu
@pytest.mark.parametrize("rate,fps", TINY_PAIRS)
def test_tiny_and_empty_spans(A, ctx, rate, fps):
    for ch in TINY_CHANNELS:
        tl = tiny_timeline(rate, fps, ch)
        al = tl.make(A, ctx)
        pcm = noise(300 + rate + ch, tl.num_samples, ch)
        want = want_of(tl, pcm, 0, TINY_FRAMES)
        empty = [n for n in range(TINY_FRAMES) if tl.b(n + 1) == tl.b(n)]
        assert not want[empty].any()
        for base in TINY_BASES:
            got = run_cover(ctx, al, tl, pcm, 0, 0, TINY_FRAMES, base)
            assert np.array_equal(got, want), (ch, base, np.argwhere(got != want)[:4].tolist())
            assert not got[empty].any() and got[:, 0].max() < SENTINEL
        if empty:
            # a batch of nothing but an empty span inside the timeline: no PCM at all, a zero record
            n = empty[len(empty) // 2]
            assert 0 < tl.b(n) < tl.num_samples
            assert not run_cover(ctx, al, tl, pcm, 0, n, 1, 3).any()


# ---- d. every channel count -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("channels", range(1, 9))
def test_every_channel_count(A, ctx, channels):
    tl = Timeline(8000, channels, (25, 1), 13 * 320)
    pcm = noise(400 + channels, tl.num_samples, channels)
    want = want_of(tl, pcm, 0, 13)
    al = tl.make(A, ctx)
    for base in (0, 1):
        got = run_cover(ctx, al, tl, pcm, 0, 0, 13, base)
        for i in range(13):
            assert np.array_equal(got[i], want[i]), (channels, base, i)
        assert np.all(got[:, 3] == 320 * channels) and got[:, 0].max() < SENTINEL


# ---- e. far into the timeline ---------------------------------------------------------------------------------------------------------
FAR_FIRST, FAR_FRAMES = 2_000_000_000, 9
FAR = Timeline(48000, 2, (30000, 1001), AC.frame_start(FAR_FIRST + FAR_FRAMES - 1, 48000, 30000, 1001) + 700)


def test_far_case_list():
    assert FAR_FRAMES % 4 != 0
    last = FAR_FIRST + FAR_FRAMES - 1
    assert AC.frame_start(last, 48000, 30000, 1001) < FAR.num_samples < AC.frame_start(last + 1, 48000, 30000, 1001)
    assert FAR.b(FAR_FIRST) > 1 << 41 and (FAR_FIRST + FAR_FRAMES) * 48000 * 1001 > 1 << 56


@gpu
def test_far_into_the_timeline(A, ctx):
    pcm_first = FAR.b(FAR_FIRST)
    cover = FAR.b(FAR_FIRST + FAR_FRAMES) - pcm_first
    assert cover == FAR.num_samples - pcm_first                                     # the tensor holds the cover and nothing else
    window = noise(51, cover, 2)
    al = FAR.make(A, ctx)
    assert al.frame_start(FAR_FIRST) == pcm_first
    for base in (0, 5):
        got = run_cover(ctx, al, FAR, window, pcm_first, FAR_FIRST, FAR_FRAMES, base)
        want = AC.levels_ref_window(window, pcm_first, 48000, 2, 30000, 1001, FAR.num_samples, FAR_FIRST, FAR_FRAMES)
        assert np.array_equal(got, want)
        assert int(got[-1, 3]) == 700 * 2 and int(got[:, 3].sum()) == cover * 2 and got[:, 0].max() < SENTINEL


@gpu
def test_far_refusals_leave_the_output_alone(A, ctx):
    import torch
    pcm = torch.zeros(64, dtype=torch.int16, device="cuda")
    out = torch.full((4, 4), -5, dtype=torch.int64, device="cuda")
    al = A.AudioLevels(ctx, 48000, 2, 30000, 1001, 1000)
    with pytest.raises(A.AmtError, match="frame range beyond 2\\^31 frames"):
        al.run_device(pcm, 0, 2 ** 31 - 1 - 3, 4, out=out)                          # first_frame + nframes == 2^31
    ctx.synchronize()
    assert bool((out == -5).all())
    big = 2 ** 31 - 1
    huge = A.AudioLevels(ctx, big, 2, 30000, big, 1000)                             # sample_rate * fps_den is almost 2^62: frame 3 is past 2^63
    assert huge.frame_start(1) == big * big // 30000 and huge.frame_start(3) == -1
    with pytest.raises(A.AmtError, match="beyond what 64-bit sample positions hold"):
        huge.run_device(pcm, 0, 3, 1, out=out)
    with pytest.raises(A.AmtError, match="beyond what 64-bit sample positions hold"):
        huge.run_device(pcm, 0, 0, 3, out=out)                                      # the END of the batch is frame 3's start
    ctx.synchronize()
    assert bool((out == -5).all())
    al.run_device(pcm, 0, 2 ** 31 - 1 - 4, 4, out=out)                              # first_frame + nframes == 2^31 - 1 is taken: frames
    ctx.synchronize()                                                               # behind the timeline, zero records
    assert not out.cpu().numpy().any()


# ---- f. one launch equals many --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("L", (8 * 512 + 1, 8 * 512 + 7))
def test_one_launch_equals_many(A, ctx, L):
    tl = sweep_timeline(L)
    al = tl.make(A, ctx)
    pcm = noise(600 + L, tl.num_samples, 1)
    whole = run_cover(ctx, al, tl, pcm, 0, 0, SWEEP_FRAMES, 1)
    assert np.array_equal(whole, want_of(tl, pcm, 0, SWEEP_FRAMES))
    singles = np.concatenate([run_cover(ctx, al, tl, pcm, 0, n, 1, 1) for n in range(SWEEP_FRAMES)])
    assert np.array_equal(singles, whole)
    parts, n = [], 0
    for k in (3, 4, 9):
        parts.append(run_cover(ctx, al, tl, pcm, 0, n, k, 1))          # each call gets exactly its own cover
        n += k
    assert n == SWEEP_FRAMES and np.array_equal(np.concatenate(parts), whole)
