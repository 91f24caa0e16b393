"""GPU parity of scan_border_kernel and scan_accumulate_kernel (LogoScan::AddFrame) on the shapes and depths their loops special-case:
odd chroma sizes, rectangles wider than one trip of the x loops and taller than one trip of the border's y loop, the 2x2 rectangle with
its one-row chroma plane, the frame corners, 8 / 10 / 12 bits (256-, 1024- and 4096-bin histograms), the `abs(min - max) <= thy` edge
from both sides, several chunks of accepted frames with a ragged last one, and container values above the declared depth.
`valid` and the integer sums are compared byte for byte with tests/scan_ref.py, the numpy statement of the reference's AddFrame."""
import numpy as np
import pytest

import scan_ref
from scan_clips import make_scan_clip
from test_gpu_parity import gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

# name: (W, H, (x, y, w, h))
RECTS = {
    "96x48_baseline": (352, 240, (224, 18, 96, 48)),
    "98x50_odd_chroma": (352, 240, (224, 18, 98, 50)),
    "520x18_three_x_trips": (720, 480, (160, 64, 520, 18)),
    "34x520_two_y_trips": (720, 576, (64, 32, 34, 520)),
    "2x2_one_row_chroma": (352, 240, (102, 54, 2, 2)),
}


def to_device(gpu, clip, W, H, bits):
    from amatsukaze_amd import DeviceClip
    torch = gpu["torch"]
    if bits <= 8:
        planes = [torch.from_numpy(clip[k]).to(gpu["dev"]) for k in "YUV"]
    else:
        planes = [torch.from_numpy(clip[k].view(np.int16)).to(gpu["dev"]) for k in "YUV"]
    return DeviceClip(*planes, width=W, height=H, bits=bits)


def ref_add(acc, clip, rect, max_valid=1 << 30):
    """the frames of clip offered to a scan_ref.ScanAccumulator in stream order, at most max_valid accepted -> the valid array"""
    x0, y0 = rect[0], rect[1]
    Y, U, V = clip["Y"], clip["U"], clip["V"]
    valid, n = np.zeros(Y.shape[0], np.uint8), 0
    for i in range(Y.shape[0]):
        if n >= max_valid:
            break
        if acc.add(Y[i, y0:, x0:], U[i, y0 // 2:, x0 // 2:], V[i, y0 // 2:, x0 // 2:]):
            valid[i] = 1
            n += 1
    return valid


def check(gpu, clip, W, H, bits, rect, thy):
    """one LogoScan over the whole clip == scan_ref; returns the valid array"""
    from amatsukaze_amd import LogoScan
    acc = scan_ref.ScanAccumulator(rect[2], rect[3], thy)
    want = ref_add(acc, clip, rect)
    scan = LogoScan(gpu["ctx"], rect[2], rect[3], thy)
    valid, nacc = scan.add_batch(to_device(gpu, clip, W, H, bits), rect[0], rect[1])
    assert valid.tobytes() == want.tobytes(), (valid.tolist(), want.tolist())
    assert nacc == int(want.sum()) == scan.nframes == acc.nframes
    s, p = scan.sums()
    ws, wp = acc.sums()
    assert p.tobytes() == wp.tobytes(), (p, wp)
    assert s.tobytes() == ws.tobytes(), np.flatnonzero(s != ws)[:8]
    return valid


def edge_plan(rng, bits, thy, n_random):
    """the frames every parametrisation holds: spread exactly thy (accepted), exactly thy + 1 in luma only, in V only and in U only
    (rejected), a border that ends at the top of the depth and one that starts at 0, then random spreads up to thy"""
    maxv = (1 << bits) - 1
    le = lambda: int(rng.randint(0, thy + 1))
    plan = [dict(spread=(thy, thy, thy)),
            dict(spread=(thy + 1, le(), le())),
            dict(spread=(le(), le(), thy + 1)),
            dict(spread=(le(), thy + 1, le())),
            dict(spread=(thy, thy, thy), base=(maxv - thy,) * 3),
            dict(spread=(thy, thy, thy), base=(0, 0, 0)),
            dict(spread=(thy + 1, thy, thy), base=(maxv - thy - 1, maxv - thy, maxv - thy))]
    kinds = [1, 0, 0, 0, 1, 1, 0]
    for _ in range(n_random):
        plan.append(dict(spread=(max(le(), min(1, thy)), le(), le())))
        kinds.append(1)
    return plan, kinds


@pytest.mark.parametrize("pad", [0, 32])
@pytest.mark.parametrize("thy", [0, 12, 40])
@pytest.mark.parametrize("bits", [8, 10, 12])
@pytest.mark.parametrize("name", sorted(RECTS))
def test_scan_shapes_exact(gpu, name, bits, thy, pad):
    W, H, rect = RECTS[name]
    rng = np.random.RandomState(1009 * sorted(RECTS).index(name) + 31 * bits + 7 * thy + pad)
    plan, kinds = edge_plan(rng, bits, thy, 13)
    clip, info = make_scan_clip(rng, W, H, pad, bits, rect, plan)
    valid = check(gpu, clip, W, H, bits, rect, thy)
    # the generator's realised spreads decide: on the edge is accepted, one past it is rejected
    assert valid.tolist() == [int(all(sp <= thy for _, sp in rec)) for rec in info]
    multi = rect[2] > 2 or rect[3] > 2                   # (a 2x2 rectangle's chroma ring is one sample: only luma can reject it)
    want_kinds = kinds if multi else [1, 0, 1, 1, 1, 1, 0] + kinds[7:]
    assert valid.tolist() == want_kinds
    if thy >= 12:
        # trimmed sums on both sides of the .5 rounding: the backgrounds do not all sit at the same offset from the ring's base
        x0, y0, w, h = rect
        offs = set()
        for i in np.flatnonzero(valid):
            bg = scan_ref.add_frame(clip["Y"][i, y0:, x0:], clip["U"][i, y0 // 2:, x0 // 2:], clip["V"][i, y0 // 2:, x0 // 2:], w, h, thy)
            offs.add(bg[0] - info[i][0][0])
        assert len(offs) > 1, offs


@pytest.mark.parametrize("bits", [8, 12])
@pytest.mark.parametrize("w,h", [(96, 48), (2, 2)])
@pytest.mark.parametrize("corner", ["origin", "bottom_right"])
def test_scan_rectangle_at_the_frame_corners(gpu, corner, w, h, bits):
    """(0, 0), and flush with the last sample of an unpadded frame"""
    W, H, thy = 352, 240, 12
    rect = (0, 0, w, h) if corner == "origin" else (W - w, H - h, w, h)
    rng = np.random.RandomState(77 + w + bits + len(corner))
    plan, kinds = edge_plan(rng, bits, thy, 5)
    clip, info = make_scan_clip(rng, W, H, 0, bits, rect, plan)
    valid = check(gpu, clip, W, H, bits, rect, thy)
    assert valid.tolist() == [int(all(sp <= thy for _, sp in rec)) for rec in info] and 0 < valid.sum() < len(plan)


def counted_plan(rng, n, thy, reject_every):
    le = lambda: int(rng.randint(0, thy + 1))
    return [dict(spread=(le(), thy + 1, le())) if i % reject_every == reject_every - 1 else dict(spread=(le(), le(), le())) for i in range(n)]


@pytest.mark.parametrize("bits,n,reject_every,want_acc", [(10, 150, 3, 100), (8, 700, 7, 600)])
def test_scan_many_accepted_frames(gpu, bits, n, reject_every, want_acc):
    """the accumulate kernel splits the accepted frames over workgroups: 100 accepted = 32 + 32 + 32 + 4; 600 accepted make the chunk
    grow to 38 frames with a last chunk of 30"""
    W, H, rect, thy = 128, 64, (38, 14, 50, 26), 12
    rng = np.random.RandomState(n)
    clip, _ = make_scan_clip(rng, W, H, 0, bits, rect, counted_plan(rng, n, thy, reject_every))
    valid = check(gpu, clip, W, H, bits, rect, thy)
    nacc = int(valid.sum())
    assert nacc == want_acc and nacc % 32 != 0
    assert (33 <= nacc <= 512) if n == 150 else nacc > 512


def test_scan_two_batches_carry_over_and_cut_in_stream_order(gpu):
    from amatsukaze_amd import LogoScan
    W, H, rect, thy, bits = 352, 240, (224, 18, 98, 50), 12, 10
    rng = np.random.RandomState(4242)
    c1, _ = make_scan_clip(rng, W, H, 32, bits, rect, counted_plan(rng, 23, thy, 4))
    c2, _ = make_scan_clip(rng, W, H, 32, bits, rect, counted_plan(rng, 31, thy, 3))
    acc = scan_ref.ScanAccumulator(rect[2], rect[3], thy)
    w1 = ref_add(acc, c1, rect)
    w2 = ref_add(acc, c2, rect, max_valid=9)
    assert w2.sum() == 9 and np.flatnonzero(w2)[-1] < 20 and w1.sum() == 18         # two of every three later frames would be valid too
    scan = LogoScan(gpu["ctx"], rect[2], rect[3], thy)
    v1, n1 = scan.add_batch(to_device(gpu, c1, W, H, bits), rect[0], rect[1])
    v2, n2 = scan.add_batch(to_device(gpu, c2, W, H, bits), rect[0], rect[1], max_valid=9)
    assert v1.tobytes() == w1.tobytes() and v2.tobytes() == w2.tobytes()
    assert n1 == w1.sum() and n2 == 9 and scan.nframes == n1 + 9
    s, p = scan.sums()
    ws, wp = acc.sums()
    assert p.tobytes() == wp.tobytes() and s.tobytes() == ws.tobytes()


def test_scan_10bit_container_values_above_the_depth(gpu):
    """AddFrame is a template over pixel_t: a border sample counts at its container value, whatever depth the clip declares.  A single
    3000 among 1020s is a spread of 1980 (rejected at thy = 12), and a border that lies in [3000, 3012] throughout is accepted with a
    background near 3000."""
    W, H, rect, thy, bits = 352, 240, (224, 18, 98, 50), 12, 10
    x0, y0, w, h = rect
    rng = np.random.RandomState(3000)
    plan = [dict(spread=(12, 7, 3)),
            dict(spread=(3, 2, 2), base=(1020, 500, 500)),           # + one luma border sample at 3000, below
            dict(spread=(12, 12, 12), base=(3000, 3000, 3000)),
            dict(spread=(5, 12, 4), base=(100, 3000, 200)),           # out of range in U only
            dict(spread=(13, 12, 12), base=(3000, 3000, 3000)),       # out of range and one past the edge
            dict(spread=(2, 3, 3), base=(600, 1020, 1021)),           # + one V border sample at 1500 (left column)
            dict(spread=(12, 0, 6), base=(32767 - 12, 32767, 20000)),
            dict(spread=(4, 4, 4))]
    clip, info = make_scan_clip(rng, W, H, 32, bits, rect, plan, container_max=32767)
    clip["Y"][1, y0, x0 + 5] = 3000
    clip["V"][5, y0 // 2 + 7, x0 // 2] = 1500
    # the interior carries out-of-range values too: the accumulate kernel sums what is there
    clip["Y"][2, y0 + 5:y0 + 9, x0 + 3:x0 + 60] = 30000
    clip["U"][3, y0 // 2 + 2, x0 // 2 + 1:x0 // 2 + 40] = 32767
    valid = check(gpu, clip, W, H, bits, rect, thy)
    assert valid.tolist() == [1, 0, 1, 1, 0, 0, 1, 1]
    bg = scan_ref.add_frame(clip["Y"][2, y0:, x0:], clip["U"][2, y0 // 2:, x0 // 2:], clip["V"][2, y0 // 2:, x0 // 2:], w, h, thy)
    assert all(3000 <= b <= 3012 for b in bg)


def test_scan_border_samples_above_32767_wrap_like_the_reference_short(gpu):
    """the reference collects the border in a std::vector<short>: 40000 enters the decision and the mean as 40000 - 65536, while
    AddScanFrame sums the real 40000"""
    W, H, rect, thy, bits = 352, 240, (224, 18, 96, 48), 12, 12
    x0, y0, w, h = rect
    rng = np.random.RandomState(40000)
    plan = [dict(spread=(9, 9, 9)), dict(spread=(12, 5, 5), base=(40000, 65535 - 5, 100)),
            dict(spread=(3, 3, 3), base=(32766, 10, 10)),             # 32766 .. 32769 straddles the wrap: a spread of 65535 as shorts
            dict(spread=(6, 6, 6))]
    clip, _ = make_scan_clip(rng, W, H, 0, bits, rect, plan, container_max=65535)
    valid = check(gpu, clip, W, H, bits, rect, thy)
    assert valid.tolist() == [1, 1, 0, 1]
    bg = scan_ref.add_frame(clip["Y"][1, y0:, x0:], clip["U"][1, y0 // 2:, x0 // 2:], clip["V"][1, y0 // 2:, x0 // 2:], w, h, thy)
    assert 40000 - 65536 <= bg[0] <= 40012 - 65536 and -6 <= bg[1] <= -1


def test_scan_thy_that_the_histogram_cannot_hold_is_refused(gpu):
    """an accepted plane spans at most thy and has to fit 1 << bits bins; 8-bit samples always do"""
    from amatsukaze_amd import LogoScan
    from amatsukaze_amd.api import AmtError
    W, H, rect = 352, 240, (224, 18, 96, 48)
    rng = np.random.RandomState(5)
    plan = [dict(spread=(200, 255, 31)), dict(spread=(0, 0, 0))]
    c8, _ = make_scan_clip(rng, W, H, 0, 8, rect, plan)
    assert check(gpu, c8, W, H, 8, rect, 300).tolist() == [1, 1]
    assert check(gpu, c8, W, H, 8, rect, 255).tolist() == [1, 1]
    assert check(gpu, c8, W, H, 8, rect, 254).tolist() == [0, 1]
    c10, _ = make_scan_clip(rng, W, H, 0, 10, rect, [dict(spread=(1023, 1000, 3))])
    assert check(gpu, c10, W, H, 10, rect, 1023).tolist() == [1]
    with pytest.raises(AmtError):
        LogoScan(gpu["ctx"], 96, 48, 1024).add_batch(to_device(gpu, c10, W, H, 10), rect[0], rect[1])
