"""frame_stats_kernel at the row widths where the dealing of (tile, lane column) pairs to the lanes can go wrong, and its one atomic per wave
and frame (lanes 0..6 add a wave's seven totals to the frame's 64-byte record with one instruction).  Row widths around one full wave
(63, 64, 65 lane columns), the flagship's 90 columns at three pitches, 96, 120 and 129 columns (32, 56 and 1 beyond a whole number of
waves), a ragged last column, 16-bit containers LSB- and MSB-aligned; heights of less than a tile, one tile to the row, and three tiles; 3
frames and 34 (one full run of 32 and a short one).  Every allocation is poisoned around its samples (tests/plane_edge_clips.py), every
batch runs without a previous frame and with one, and all eight words of every record are compared as bytes with the numpy statement
(oracle/frame_stats_oracle.py through plane_edge_clips).  The host test replays the launch geometry and the lane map themselves --
tests/cpp/stats_spans_replay.cpp includes stats_body.h -- and needs no GPU.  (The name: the file was written for a map that cuts tile
rows into 64-column spans; it was measured and not kept, profiles/stats_spans_notes.md, and the cases stay.)"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import plane_edge_clips as P
import surface_clips as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = ("DIFF_TOP", "DIFF_BOT", "VERT", "COMB", "COMB_PREV", "SUM", "VERT_PREV", "reserved")

# (name, bits, W in samples, pitch in samples)
WIDTHS = [("c63", 8, 1008, 1008), ("c64", 8, 1024, 1024), ("c65", 8, 1040, 1040),
          ("c90-p1440", 8, 1440, 1440), ("c90-p1472", 8, 1440, 1472), ("c90-p1536", 8, 1440, 1536),
          ("c96", 8, 1536, 1536), ("c120", 8, 1920, 1920), ("c129", 8, 2064, 2064), ("ragged", 8, 1450, 1472),
          ("lsb10", 10, 720, 720)]
MSB_WIDTH = ("msb10", 10, 720, 720)
HEIGHTS = (4, 5, 23, 24, 25, 49)
FRAMES = (3, 34)
CASES = [(w, H, N) for w in WIDTHS for H in HEIGHTS for N in FRAMES]
MSB_CASES = [(MSB_WIDTH, H, N) for H in HEIGHTS for N in FRAMES]


def case_id(case):
    (name, bits, W, pitch), H, N = case
    return f"{name}-h{H}-n{N}"


def col_groups(bits, W):
    return -(-W * (1 if bits <= 8 else 2) // P.COL_BYTES)


def test_case_list_is_what_it_says():
    """lane columns per row of the widths, all of them in the buffer-load forms, the ragged one in the ragged form"""
    assert [col_groups(b, W) for _, b, W, _ in WIDTHS + [MSB_WIDTH]] == [63, 64, 65, 90, 90, 90, 96, 120, 129, 91, 90, 90]
    for name, bits, W, pitch in WIDTHS + [MSB_WIDTH]:
        assert P.predicted_form("frame_stats", W, pitch, 1 if bits <= 8 else 2) == ("buf_ragged" if name == "ragged" else "buf")


# ---------------------------------------------------------------------------------------------------------------- the map, on the host
@pytest.fixture(scope="module")
def replay():
    from amatsukaze_amd import build as B
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "stats_spans_replay")
        subprocess.check_call([B.hipcc(), "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "amatsukaze_amd", "csrc"),
                               "-o", exe, os.path.join(ROOT, "tests", "cpp", "stats_spans_replay.cpp")], stderr=subprocess.DEVNULL)

        def run(es, pitch, W, H, N):
            rows = [[int(x) for x in l.split()] for l in subprocess.check_output([exe, *map(str, (es, pitch, W, H, N))], text=True).splitlines()]
            gx, gy, cols, buf, ragged, tile_rows = rows[0]
            return dict(gx=gx, gy=gy, cols=cols, buf=buf, ragged=ragged, tile_rows=tile_rows, lanes=np.array(rows[1:], np.int64))
        yield run


@pytest.mark.parametrize("width", WIDTHS + [MSB_WIDTH], ids=lambda w: w[0])
def test_every_column_of_every_tile_has_one_lane_and_no_lane_idles(replay, width):
    name, bits, W, pitch = width
    es = 1 if bits <= 8 else 2
    for H in HEIGHTS + (240, 1080):                 # (more tiles than the GPU cases: waves that straddle tiles at every phase)
        for N in FRAMES:
            r = replay(es, pitch, W, H, N)
            C, T = col_groups(bits, W), -(-H // r["tile_rows"])
            assert (r["cols"], r["buf"], r["gy"]) == (C, 1, -(-N // P.RUN)) and r["gx"] % 8 == 0
            wave, tile, col = r["lanes"].T
            assert len(wave) == r["gx"] * 128 and np.array_equal(np.bincount(wave), np.full(r["gx"] * 2, 64))
            assert tile.min() >= 0 and col.min() >= 0
            busy = (tile < T) & (col < C)
            # a lane without pixels stands past the last tile (the kernel tells it by its tile alone)
            assert np.all(tile[~busy] >= T)
            owners = np.bincount(tile[busy] * C + col[busy], minlength=T * C)
            assert owners.shape == (T * C,) and np.all(owners == 1), f"{name} H {H}: columns with {set(owners.tolist())} owners"
            # no lane of a wave before the last wave with pixels is idle
            last = wave[busy].max()
            assert np.all(busy[wave < last]), f"{name} H {H}: idle lanes in waves {sorted(set(wave[(wave < last) & ~busy].tolist()))[:5]}"
            # XCD k (workgroups k, k + 8, ...) holds one contiguous stretch of the order of waves
            per = r["gx"] // 8
            for k in range(8):
                w = np.unique(wave.reshape(r["gx"], 128)[k::8])
                assert np.array_equal(w, np.arange(2 * k * per, 2 * (k + 1) * per))


# ---------------------------------------------------------------------------------------------------------------- the records, on the GPU
@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return dict(torch=torch, ctx=Context(0), dev=torch.device("cuda:0"))


def assert_records(got, want, what):
    assert got.dtype == want.dtype == np.uint64 and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        n, k = bad[0]
        raise AssertionError(f"{what}: {len(bad)} words differ, first frame {n} {WORDS[k]}: got {got[n, k]}, want {want[n, k]}; "
                             f"words off: {sorted({WORDS[j] for j in bad[:, 1]})}")


def device_metrics(gpu, fs, t, prevY=None):
    torch = gpu["torch"]
    out = torch.full((t.shape[0], 8), -1, dtype=torch.int64, device=gpu["dev"])
    fs.run_device(t, out, prevY=prevY)
    gpu["ctx"].synchronize()
    return out.cpu().numpy().astype(np.uint64)


def samples_of(case, seed=0):
    (name, bits, W, pitch), H, N = case
    rng = np.random.default_rng([bits, W, pitch, H, N, seed])
    dt = P.dtype_of(bits)
    return rng.integers(0, int(np.iinfo(dt).max) + 1, (N + 1, H, W)).astype(dt)             # (the whole container, as plane_edge_clips does)


def check(gpu, case, base_bytes=0):
    """frames 1..N of a poisoned allocation, without a previous frame and with frame 0 as the previous frame"""
    from amatsukaze_amd import FrameStats
    (name, bits, W, pitch), H, N = case
    clip = P.embed(samples_of(case), pitch, base=base_bytes // (1 if bits <= 8 else 2))
    t = P.to_device(gpu["torch"], gpu["dev"], clip)
    assert t.data_ptr() % 256 == base_bytes
    fs = FrameStats(gpu["ctx"], W, H, bits)
    batch = clip.sub(1)
    assert_records(device_metrics(gpu, fs, t[1:]), P.true_metrics(batch), case_id(case) + " no previous frame")
    assert_records(device_metrics(gpu, fs, t[1:], t[0]), P.true_metrics(batch, clip.sub(0, 1)), case_id(case) + " with a previous frame")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_records(gpu, case):
    check(gpu, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(w, 49, N) for w in WIDTHS for N in FRAMES], ids=case_id)
def test_records_with_the_base_16_bytes_in(gpu, case):
    """every row starts 16 bytes off the allocation: no wave starts on a 128-byte line any more, and nothing else may change"""
    check(gpu, case, base_bytes=16)


@pytest.mark.gpu
@pytest.mark.parametrize("case", MSB_CASES, ids=case_id)
def test_records_msb(gpu, case):
    """the MSB form: P010-like surfaces, random low bits under the samples, the previous picture in front of the batch"""
    from amatsukaze_amd import DeviceSurfaces, FrameStats
    (name, bits, W, pitch), H, N = case
    rng = np.random.default_rng([bits, W, H, N])
    clip = P.embed(SC.msb_containers(rng.integers(0, 1 << bits, (N + 1, H, W)), bits, rng), pitch, rows_after=2)
    t = P.to_device(gpu["torch"], gpu["dev"], clip)
    fs = FrameStats(gpu["ctx"], W, H, bits)
    surf = lambda x: DeviceSurfaces(x, None, None, W, H, bits, interleaved=True, msb=True)
    shift = 16 - bits
    frames = clip.frames() >> shift
    for prev, dprev in ((None, None), (frames[0], surf(t[0:1]))):
        out = gpu["torch"].full((N, 8), -1, dtype=gpu["torch"].int64, device=gpu["dev"])
        fs.run_device_surfaces(surf(t[1:]), out, dprev)
        gpu["ctx"].synchronize()
        assert_records(out.cpu().numpy().astype(np.uint64), P.FS.frame_metrics(frames[1:], prev),
                       case_id(case) + (" no previous picture" if prev is None else " with a previous picture"))


def top_value_records(top, W, H, N):
    """every sample of N frames at `top`, the frame before them all zero, written out by hand: frame 0 differs from the frame before in
    every sample and its weave (even rows top, odd rows 0) sets every inner row against two neighbours of the other value; from frame
    1 on nothing differs from anything.  No row differs from the row two below it"""
    rec = np.zeros((N, 8), np.uint64)
    rec[:, 5] = top * W * H
    rec[0, 0], rec[0, 1], rec[0, 4] = top * W * -(-H // 2), top * W * (H // 2), top * W * (H - 2)
    return rec


TOP_CASES = [(("c90-p1472", 8, 1440, 1472), 49, 34), (("lsb15", 15, 720, 736), 49, 34)]


def test_top_value_closed_forms_are_the_oracles():
    for (name, bits, W, pitch), H, N in TOP_CASES:
        top = int(np.iinfo(P.dtype_of(bits)).max)
        Y = np.full((N, H, W), top, P.dtype_of(bits))
        assert np.array_equal(P.FS.frame_metrics(Y, np.zeros((H, W), Y.dtype)), top_value_records(top, W, H, N))
        # (a wave's largest total fits the 32 bits it is carried in, and the seven words of frame 0 that are not zero are four)
        assert 64 * 24 * 16 * 255 < 2 ** 32 and 64 * 16 * 8 * 65535 < 2 ** 32


@pytest.mark.gpu
@pytest.mark.parametrize("case", TOP_CASES, ids=case_id)
def test_every_sample_at_its_top_value(gpu, case):
    """every wave's totals at their largest, seven lanes of every wave adding at once to one record: nothing is lost"""
    from amatsukaze_amd import FrameStats
    (name, bits, W, pitch), H, N = case
    dt = P.dtype_of(bits)
    top = int(np.iinfo(dt).max)
    clip = P.embed(np.concatenate([np.zeros((1, H, W), dt), np.full((N, H, W), top, dt)]), pitch)
    t = P.to_device(gpu["torch"], gpu["dev"], clip)
    fs = FrameStats(gpu["ctx"], W, H, bits)
    assert_records(device_metrics(gpu, fs, t[1:], t[0]), top_value_records(top, W, H, N), case_id(case))
