"""The audio level kernel against numpy (tests/audio_clips.py levels_ref), byte for byte.  Every case is tens of video frames but the
last, which needs more than the 4 096 frames run_amts reads at a time."""
import numpy as np
import pytest

import audio_clips as AC

pytestmark = pytest.mark.gpu

NTSC = (30000, 1001)


@pytest.fixture(scope="module")
def A():
    import amatsukaze_amd
    return amatsukaze_amd


@pytest.fixture(scope="module")
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


def noise(rng, samples, channels):
    x = rng.integers(-32768, 32768, (samples, channels)).astype(np.int16)
    x.reshape(-1)[[3, samples * channels // 2]] = (-32768, 32767)          # the extremes, planted
    return x


def device_run(A, ctx, al, flat, offset, count, pcm_first, first_frame, nframes):
    """records of [first_frame, first_frame + nframes) from the device tensor `flat`, whose elements [offset, offset + count * channels)
    are sample-frames pcm_first .. of the timeline"""
    view = flat[offset:offset + count * al.channels]
    out = al.run_device(view, pcm_first, first_frame, nframes)
    ctx.synchronize()
    return out.cpu().numpy().astype(np.uint64)


def test_basic_48k_stereo(A, ctx):
    rate, ch, n = 48000, 2, 37
    ns = AC.frame_start(n, rate, *NTSC)                                     # the buffer is exactly the timeline
    pcm = noise(np.random.default_rng(1), ns, ch)
    al = A.AudioLevels(ctx, rate, ch, *NTSC, ns)
    assert [al.frame_start(k) for k in (0, 1, 2, n)] == [AC.frame_start(k, rate, *NTSC) for k in (0, 1, 2, n)] and al.num_frames() == n
    got = al.run(pcm)
    want = AC.levels_ref(pcm, rate, ch, *NTSC, ns, 0, n)
    assert got.shape == (n, 4) and got.dtype == np.uint64
    assert np.array_equal(got, want)
    assert want[:, 0].max() == 32768 and int(want[:, 3].sum()) == ns * ch


def test_alignment_44k_mono(A, ctx):
    import torch
    rate, ch, n, fps = 44100, 1, 23, (24000, 1001)
    ns = AC.frame_start(n, rate, *fps)
    pcm = noise(np.random.default_rng(2), ns, ch)
    host = np.full(ns + 9, 32767, np.int16)
    host[1:1 + ns] = pcm.reshape(-1)
    flat = torch.from_numpy(host).cuda()
    base = flat.data_ptr() + 2                                              # one element past the tensor's base
    assert flat.data_ptr() % 16 == 0
    starts = {(base + 2 * ch * AC.frame_start(k, rate, *fps)) % 16 for k in range(n)}
    ends = {(base + 2 * ch * AC.frame_start(k + 1, rate, *fps)) % 16 for k in range(n)}
    assert starts == set(range(0, 16, 2)) and ends == set(range(0, 16, 2))      # every even misalignment of a span's start and of its end
    al = A.AudioLevels(ctx, rate, ch, *fps, ns)
    got = device_run(A, ctx, al, flat, 1, ns, 0, 0, n)
    assert np.array_equal(got, AC.levels_ref(pcm, rate, ch, *fps, ns, 0, n))


def test_extremes_all_minus_32768(A, ctx):
    rate, ch, n = 48000, 2, 12
    ns = AC.frame_start(n, rate, *NTSC)
    pcm = np.full((ns, ch), -32768, np.int16)
    got = A.AudioLevels(ctx, rate, ch, *NTSC, ns).run(pcm)
    count = got[:, 3].astype(np.uint64)
    assert np.array_equal(count, np.array([(AC.frame_start(k + 1, rate, *NTSC) - AC.frame_start(k, rate, *NTSC)) * ch for k in range(n)], np.uint64))
    assert np.all(got[:, 0] == 32768) and np.array_equal(got[:, 1], count * np.uint64(32768)) and np.array_equal(got[:, 2], count << np.uint64(30))
    assert np.array_equal(got, AC.levels_ref(pcm, rate, ch, *NTSC, ns, 0, n))


def test_end_of_the_timeline(A, ctx):
    import torch
    rate, ch, k = 48000, 2, 9
    ns = AC.frame_start(k, rate, *NTSC) + 700                               # ends inside frame k's span; the video goes on for five frames
    n = k + 1 + 5
    host = np.full((AC.frame_start(n, rate, *NTSC), ch), 32767, np.int16)       # beyond num_samples: 32767, which must not count
    host[:ns] = noise(np.random.default_rng(4), ns, ch) // 2                # (below 32767 everywhere inside the timeline)
    flat = torch.from_numpy(host.reshape(-1)).cuda()
    al = A.AudioLevels(ctx, rate, ch, *NTSC, ns)
    assert al.num_frames() == k + 1
    got = device_run(A, ctx, al, flat, 0, host.shape[0], 0, 0, n)
    assert np.array_equal(got, AC.levels_ref(host, rate, ch, *NTSC, ns, 0, n))
    assert int(got[k, 3]) == 700 * ch and np.all(got[k + 1:] == 0) and got[:k + 1, 0].max() < 32767
    # frames that lie wholly behind the timeline need no PCM at all
    tail = al.run_device(flat[:0], 0, k + 1, 5)
    ctx.synchronize()
    assert not tail.cpu().numpy().any()


def test_chunks_and_surroundings(A, ctx):
    import torch
    rate, ch, n = 48000, 2, 24
    ns = AC.frame_start(n, rate, *NTSC)
    pcm = noise(np.random.default_rng(5), ns, ch) // 2                      # below 32767: a read outside a span would show in PEAK
    al = A.AudioLevels(ctx, rate, ch, *NTSC, ns)
    whole = al.run(pcm)
    assert np.array_equal(whole, AC.levels_ref(pcm, rate, ch, *NTSC, ns, 0, n)) and whole[:, 0].max() < 32767
    b = lambda f: AC.frame_start(f, rate, *NTSC)
    pad = 37                                                                # elements of 32767 in front: an odd element offset
    def surrounded(f0, f1):
        host = np.full(pad + (b(f1) - b(f0)) * ch + 64, 32767, np.int16)
        host[pad:pad + (b(f1) - b(f0)) * ch] = pcm[b(f0):b(f1)].reshape(-1)
        return torch.from_numpy(host).cuda()
    got = device_run(A, ctx, al, surrounded(5, 20), pad, b(20) - b(5), b(5), 5, 15)
    assert np.array_equal(got, whole[5:20])
    two = np.concatenate([device_run(A, ctx, al, surrounded(5, 11), pad, b(11) - b(5), b(5), 5, 6),
                          device_run(A, ctx, al, surrounded(11, 20), pad, b(20) - b(11), b(11), 11, 9)])
    assert np.array_equal(two, whole[5:20])


def test_six_channels(A, ctx):
    rate, ch, n = 48000, 6, 8
    ns = AC.frame_start(n, rate, *NTSC)
    pcm = noise(np.random.default_rng(6), ns, ch)
    got = A.AudioLevels(ctx, rate, ch, *NTSC, ns).run(pcm)
    assert np.array_equal(got, AC.levels_ref(pcm, rate, ch, *NTSC, ns, 0, n))


def test_zero_frames_and_refusals(A, ctx):
    import torch
    rate, ch, n = 48000, 2, 6
    ns = AC.frame_start(n, rate, *NTSC)
    flat = torch.from_numpy(noise(np.random.default_rng(7), ns, ch).reshape(-1)).cuda()
    al = A.AudioLevels(ctx, rate, ch, *NTSC, ns)
    out = torch.full((n, 4), -5, dtype=torch.int64, device="cuda")
    assert al.run_device(flat, 0, 2, 0, out=out) is out                     # nframes == 0: returns 1 ...
    ctx.synchronize()
    assert bool((out == -5).all())                                          # ... and writes nothing
    b = lambda f: AC.frame_start(f, rate, *NTSC)
    with pytest.raises(A.AmtError, match="does not cover"):                 # one sample-frame short at the end of the required cover
        al.run_device(flat[:(b(4) - 1) * ch], 0, 0, 4)
    with pytest.raises(A.AmtError, match="does not cover"):                 # ... and at its start
        al.run_device(flat[(b(2) + 1) * ch:], b(2) + 1, 2, 4)
    al.run_device(flat[b(2) * ch:b(4) * ch], b(2), 2, 2)                    # the exact cover is taken
    with pytest.raises(A.AmtError, match="negative"):
        al.run_device(flat, 0, -1, 2)
    ctx.synchronize()
    for bad in (dict(channels=0), dict(channels=9), dict(fps_num=0)):
        args = dict(sample_rate=rate, channels=ch, fps_num=NTSC[0], fps_den=NTSC[1], num_samples=ns)
        args.update(bad)
        with pytest.raises(A.AmtError, match=r"\[AudioLevels\]"):
            A.AudioLevels(ctx, **args)


def test_end_to_end_amts(A, ctx, tmp_path):
    clip, nframes = AC.e2e_clip(tmp_path)
    amts = A.AmtsFile(clip.amtspath, ctx)
    spf, ns = amts.audio_info()
    assert (spf, ns) == (clip.spf, clip.num_samples)
    al = A.AudioLevels(ctx, AC.E2E_RATE, 2, *AC.E2E_FPS, ns)
    assert al.num_frames() == nframes
    got = al.run_amts(amts)
    assembled = AC.get_audio_ref(clip.wave, clip.frames, 0, ns)
    want = al.run(assembled)
    assert np.array_equal(want, AC.levels_ref(assembled, AC.E2E_RATE, 2, *AC.E2E_FPS, ns, 0, nframes))
    assert np.array_equal(got, want)
    assert np.array_equal(al.run_amts(amts, clip.wavpath, first_frame=7, nframes=30), want[7:37])
    assert A.mute_sections(got) == AC.E2E_SECTIONS == AC.mute_sections_ref(want, 50, 10)
    # frames behind the timeline: zero records
    more = al.run_amts(amts, nframes=nframes + 4)
    assert np.array_equal(more[:nframes], want) and not more[nframes:].any()
    with pytest.raises(A.AmtError, match="2 channels"):
        A.AudioLevels(ctx, AC.E2E_RATE, 1, *AC.E2E_FPS, ns).run_amts(amts, nframes=4)
    with pytest.raises(A.AmtError, match="failed to open"):
        al.run_amts(amts, str(tmp_path / "absent.wav"))


def test_amts_in_more_than_one_chunk(A, ctx, tmp_path):
    """run_amts cuts the clip into chunks of 4096 video frames: a clip a little longer than one chunk against one call on the assembled
    audio (whose kernel the tests above pin to numpy)"""
    nvideo = 4096 + 37
    naudio = -(-AC.frame_start(nvideo, AC.E2E_RATE, *AC.E2E_FPS) // 1024)
    clip = AC.AudioClip(tmp_path, naudio=naudio, spf=1024, seed=9, sample_rate=AC.E2E_RATE, name="long")
    amts = A.AmtsFile(clip.amtspath, ctx)
    al = A.AudioLevels(ctx, AC.E2E_RATE, 2, *AC.E2E_FPS, clip.num_samples)
    got = al.run_amts(amts)
    assert got.shape[0] == al.num_frames() > 4096
    assert np.array_equal(got, al.run(clip.timeline))
    lo, hi = AC.frame_start(4090, AC.E2E_RATE, *AC.E2E_FPS), AC.frame_start(4102, AC.E2E_RATE, *AC.E2E_FPS)
    assert np.array_equal(got[4090:4102], AC.levels_ref(clip.timeline, AC.E2E_RATE, 2, *AC.E2E_FPS, clip.num_samples, 4090, 12)) and hi > lo
