"""frame_stats_kernel and logofind_kernel at the edges of their addressing: rows that are no multiple of the load size through the raw
buffer loads, gaps between frames, offset bases, a previous frame in another allocation, heights around the tile height (4, 5 and odd
ones included), every byte count of the ragged dword, frame runs of 1 .. 65 frames, tile counts that leave workgroups idle, and
16-bit containers over their whole range -- all byte-equal to the numpy statements (oracle/frame_stats_oracle.py,
tests/logofind_ref.py).  Everything around the frames holds the top value, so a read outside `height * pitch` bytes of a frame, or
of a row's padding, shows.  tests/test_plane_edge_inputs_host.py shows for every input here which wrong kernels it would catch."""
import numpy as np
import pytest

import plane_edge_clips as P

pytestmark = pytest.mark.gpu

WORDS = ("DIFF_TOP", "DIFF_BOT", "VERT", "COMB", "COMB_PREV", "SUM", "VERT_PREV", "reserved")


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return dict(torch=torch, ctx=Context(0), dev=torch.device("cuda:0"))


def device_metrics(gpu, fs, t, prevY=None):
    torch = gpu["torch"]
    out = torch.full((t.shape[0], 8), -1, dtype=torch.int64, device=gpu["dev"])
    fs.run_device(t, out, prevY=prevY)
    gpu["ctx"].synchronize()
    return out.cpu().numpy().astype(np.uint64)


def assert_records(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        n, k = bad[0]
        raise AssertionError(f"{what}: {len(bad)} words differ, first frame {n} {WORDS[k]}: got {got[n, k]}, want {want[n, k]}; "
                             f"words off: {sorted({WORDS[j] for j in bad[:, 1]})}")


def check_frame_metrics(gpu, family, case, closed_form=None):
    """the batch (frames 1..N of the allocation) without a previous frame, and with one: frame 0 of the allocation, or the family's
    separate allocation"""
    from amatsukaze_amd import FrameStats
    bits, W, pitch, H, N, kw = case
    clip, sep = P.fs_clip(case, family)
    batch = clip.sub(1)
    t = P.to_device(gpu["torch"], gpu["dev"], clip)
    assert (t.storage_offset(), t.stride(0), t.stride(1), W, t.shape[1], t.shape[0]) == clip.view() and t.shape[2] == pitch
    fs = FrameStats(gpu["ctx"], W, H, bits)
    want = P.true_metrics(batch) if closed_form is None else closed_form(batch.top, W, H, N, False)
    assert_records(device_metrics(gpu, fs, t[1:]), want, P.case_id(case) + " no previous frame")
    if sep is not None:
        prev, prevY = sep, P.to_device(gpu["torch"], gpu["dev"], sep)[0]
    else:
        prev, prevY = clip.sub(0, 1), t[0]
    want = P.true_metrics(batch, prev) if closed_form is None else closed_form(batch.top, W, H, N, True)
    assert_records(device_metrics(gpu, fs, t[1:], prevY), want, P.case_id(case) + " with a previous frame")


def test_parameter_lists_reach_every_form():
    """(the forms as tests/plane_edge_clips.py predicts them from the launchers' rules)"""
    assert P.forms_reached("frame_stats", P.GEOMETRY_CASES) == P.FRAME_STATS_FORMS
    assert P.forms_reached("frame_stats", P.ADDRESSING_CASES) == P.FRAME_STATS_FORMS
    unaligned = [(8, W, p) for W, p in P.UNALIGNED_8] + [(10, W, p) for W, p in P.UNALIGNED_16]
    assert P.forms_reached("frame_stats", unaligned) == {(f, es) for f in ("buf", "buf_ragged") for es in (1, 2)}
    assert P.forms_reached("frame_stats", P.BATCH_CASES) == {("buf", 1), ("buf_ragged", 1)}
    assert P.forms_reached("logofind", P.LOGOFIND_CASES) == P.LOGOFIND_FORMS


@pytest.mark.parametrize("case", P.GEOMETRY_CASES, ids=P.case_id)
def test_frame_metrics_geometry(gpu, case):
    """one width per form and sample size; heights 4, 5 and around one and two tiles; widths 1, 2, 15, 16, 17"""
    check_frame_metrics(gpu, "geometry", case)


@pytest.mark.parametrize("case", P.ADDRESSING_CASES, ids=P.case_id)
def test_frame_metrics_addressing(gpu, case):
    """pitches that are no multiple of 16 (4, 2) bytes through the buffer loads; a base one sample in; crops out of taller, wider frames
    with everything around them poisoned"""
    check_frame_metrics(gpu, "addressing", case)


@pytest.mark.parametrize("case", P.SEPARATE_PREV_CASES, ids=P.case_id)
def test_frame_metrics_previous_frame_in_another_allocation(gpu, case):
    check_frame_metrics(gpu, "separate_prev", case)


@pytest.mark.parametrize("case", P.FULL_RANGE_8_CASES, ids=P.case_id)
def test_frame_metrics_full_range_8bit(gpu, case):
    """every vertical (a, c) pair of 8-bit samples: the whole table of v_lerp_u8 / v_sad_u8 as the kernel uses them"""
    check_frame_metrics(gpu, "full_range_8", case)


@pytest.mark.parametrize("case", P.FULL_RANGE_16_CASES, ids=P.case_id)
def test_frame_metrics_full_range_16bit_containers(gpu, case):
    """containers 0..65535 at declared depths 10, 12 and 15 (the depth selects the sample size, nothing else), with every vertical
    triple over the values around the 16-bit halves' carries, at both column parities"""
    check_frame_metrics(gpu, "full_range_16", case)


@pytest.mark.parametrize("case", P.SATURATED_CASES, ids=P.case_id)
def test_frame_metrics_saturated_against_closed_forms(gpu, case):
    """every term of every row at its maximum (a wave's largest partial, 64 * 16 * 8 * 65535, is below 2^32)"""
    from test_plane_edge_inputs_host import closed_form_records
    check_frame_metrics(gpu, "saturated", case, closed_form=closed_form_records)


@pytest.mark.parametrize("case", P.BATCH_CASES, ids=P.case_id)
def test_frame_metrics_batches(gpu, case):
    """1, 2, 31, 32, 33, 64, 65 frames: runs of 32, two frames per trip of the unragged loop"""
    check_frame_metrics(gpu, "batches", case)


@pytest.mark.parametrize("case", P.DEALING_CASES, ids=P.case_id)
def test_frame_metrics_dealing(gpu, case):
    """1, 3, 129 and 127 lane columns per row: waves that straddle tiles, workgroups of the round-up to 8 that own nothing"""
    check_frame_metrics(gpu, "dealing", case)


def device_sums(gpu, t, clip, bits, chunks):
    from amatsukaze_amd import LogoFinder
    lf = LogoFinder(gpu["ctx"], clip.W, clip.H, bits)
    for a, b in chunks:
        lf.add_device(t[a:b])
    S1, SM = lf.sums()
    assert lf.nframes == clip.N
    return np.concatenate([S1.ravel(), SM.ravel()])


@pytest.mark.parametrize("case", P.LOGOFIND_CASES, ids=P.lf_case_id)
def test_logofind_sums(gpu, case):
    """whole batch, ragged chunks and frame by frame, as tests/test_gpu_logofind.py test_sums_match_numpy does"""
    bits, w, h, pitch, n, kw = case
    clip = P.lf_clip(case)
    t = P.to_device(gpu["torch"], gpu["dev"], clip)
    want = P.true_sums(clip)
    for chunks in ([(0, n)], [(a, min(n, a + 7)) for a in range(0, n, 7)], [(i, i + 1) for i in range(n)]):
        got = device_sums(gpu, t, clip, bits, chunks)
        if got.tobytes() != want.tobytes():
            bad = np.flatnonzero(got != want)
            which, at = divmod(int(bad[0]), w * h)
            raise AssertionError(f"{P.lf_case_id(case)} in {len(chunks)} calls: {len(bad)} sums differ, first {'S1 SM'.split()[which]} at "
                                 f"(y, x) = {divmod(at, w)}: got {got[bad[0]]}, want {want[bad[0]]}")
