"""The resize on the GPU where a wave's work splits or wraps (tests/test_gpu_resize.py has the small shapes):
horizontal spans that take a second staging pass and fill the wave's LDS region to its last byte; runs of 32, 16 and 8 output columns
(resize_columns_per_wave below 64) and the create's refusal one step past the region; rows of the vertical 16-byte form that take
several chunks of 64 lanes, with a dead tail and with a partial lane in a later chunk; windows that the unrolled loops do not divide;
one Resizer used for calls of different frame counts and lane forms; and layouts of which only one side is 16-byte aligned.

Every case compares every container of the three destination buffers with tests/resize_ref.py, exactly, and states with that file's
port of the columns-per-wave rule (held against the C++ in tests/test_resize_host.py) which branch it reaches."""
import numpy as np
import pytest

import resize_ref as R
from test_gpu_resize import aligned_layouts, gpu, narrow_layouts, noise_case, run_resize  # noqa: F401  (gpu: the module's fixture)
from test_gpu_temporal_nr import Buf, check_against, download, sentinel_buf, upload

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("layouts", [aligned_layouts, narrow_layouts], ids=["aligned", "narrow"])


def aligned_to_narrow(*a):
    return aligned_layouts(*a)[0], narrow_layouts(*a)[1]


def narrow_to_aligned(*a):
    return narrow_layouts(*a)[0], aligned_layouts(*a)[1]


def rows_on_16_bytes(layouts, sw, sh, dw, dh, bits):
    """(source, destination): does every row of every plane begin on a multiple of 16 bytes of its buffer -- offset, frame stride and
    pitch, the operands of resize_vec16 (device allocations begin on far more than 16)"""
    es = 1 if bits <= 8 else 2
    sl, dl = layouts(sw, sh, dw, dh, bits)
    on16 = lambda buf: all((off * es | fs * es | p * es) % 16 == 0 for _, _, p, fs, off in buf.geom)
    return on16(Buf(2, sw, sh, bits, **sl)), on16(Buf(2, dw, dh, bits, **{k: v for k, v in dl.items() if k != "tight_end"}))


def vec_form(layouts, sw, sh, dw, dh, bits):
    """the joint lane rule: the 16-byte form where source AND destination are aligned (the intermediate, the object's own, always is)"""
    return all(rows_on_16_bytes(layouts, sw, sh, dw, dh, bits))


def cpw_of(S, D, bits, **kw):
    """(cpw, K, the runs' spans in bytes) of a luma row of S -> D and of its chroma row"""
    es = 1 if bits <= 8 else 2
    return R.columns_per_wave(S, D, es, **kw), R.columns_per_wave(S // 2, D // 2, es, **kw)


def staging_passes(span_bytes, es, vec):
    """passes of a wave's staging loop over a span: 64 lanes of 16 bytes, or of one container, per pass (the 16-byte form starts at the
    16 bytes the span begins in, which adds no pass to any span here: asserted where it matters by the span's size alone)"""
    return -(-span_bytes // (16 * 64)) if vec else -(-(span_bytes // es) // 64)


def chunks_of(W, bits):
    """(lanes, chunks of 64 lanes) of a row of W containers in the vertical stage's 16-byte form"""
    es = 1 if bits <= 8 else 2
    lanes = -(-W * es // 16)
    return lanes, -(-lanes // 64)


def case(gpu, what, n, src, dst, bits, layouts, **kw):
    planes, want = noise_case(n, src[0], src[1], dst[0], dst[1], bits)
    return run_resize(gpu, (what, bits, layouts.__name__), planes, bits, dst, layouts, want, **kw)


# ---- 1. a span that fills the region exactly; two staging passes ----
@BOTH
def test_a_span_of_exactly_the_region_at_16_bits(gpu, layouts):
    (cpw, K, spans), (cpwC, KC, spansC) = cpw_of(1000, 32, 16)
    assert (cpw, K, spans) == (64, 250, (2000,)) and (cpwC, KC, spansC) == (64, 250, (1000,))
    assert spans[0] + R.REGION_SLACK == R.REGION_BYTES                 # the limit itself
    assert R.program(8, 8)[0] == 8 and R.program(4, 4)[0] == 4          # the vertical stage copies
    vec = vec_form(layouts, 1000, 8, 32, 8, 16)
    assert vec == (layouts is aligned_layouts)
    assert (staging_passes(2000, 2, vec), staging_passes(1000, 2, vec)) == ((2, 1) if vec else (16, 8))
    case(gpu, "1000 -> 32", 2, (1000, 8), (32, 8), 16, layouts)


@BOTH
def test_a_span_of_exactly_the_region_at_8_bits_and_a_run_of_two_columns(gpu, layouts):
    (cpw, K, spans), (cpwC, KC, spansC) = cpw_of(2000, 66, 8)
    assert (cpw, K, spans) == (64, 243, (2000, 243)) and (cpwC, KC, spansC) == (64, 243, (1000,))
    assert 66 - 64 == 2                                                 # the second run's columns
    vec = vec_form(layouts, 2000, 8, 66, 8, 8)
    assert staging_passes(2000, 1, vec) == (2 if vec else 32)
    case(gpu, "2000 -> 66", 2, (2000, 8), (66, 8), 8, layouts)


# ---- 2. runs of fewer than 64 columns ----
@BOTH
def test_runs_of_32_columns_in_luma_and_64_in_chroma(gpu, layouts):
    (cpw, K, spans), (cpwC, KC, spansC) = cpw_of(1760, 66, 16)
    assert (cpw, K, max(spans), len(spans)) == (32, 214, 2000, 3) and (cpwC, KC, spansC) == (64, 214, (1760,))
    assert 66 - 2 * 32 == 2                                             # the last luma run's columns
    case(gpu, "1760 -> 66", 2, (1760, 8), (66, 8), 16, layouts)


@BOTH
def test_runs_of_8_columns_at_16_bits(gpu, layouts):
    (cpw, K, spans), (cpwC, KC, spansC) = cpw_of(2048, 32, 16)
    assert (cpw, K, max(spans), len(spans)) == (8, 512, 1920, 4) and (cpwC, KC, max(spansC), len(spansC)) == (8, 512, 1472, 2)
    assert R.program(4, 4)[0] == 4 and R.program(2, 2)[0] == 2
    case(gpu, "2048 -> 32", 2, (2048, 4), (32, 4), 16, layouts)


def test_runs_of_16_columns_at_8_bits(gpu):
    (cpw, K, spans), (cpwC, KC, spansC) = cpw_of(2048, 32, 8)
    assert (cpw, K, len(spans)) == (16, 512, 2) and (cpwC, KC, spansC) == (64, 512, (1024,))
    case(gpu, "2048 -> 32", 2, (2048, 4), (32, 4), 8, aligned_layouts)


# ---- 3. the refusal's boundary; a chroma plane of one column ----
@pytest.mark.parametrize("bits, fits, refused", [(8, 2000, 2002), (16, 1000, 1002)])
def test_the_widest_window_that_fits_and_the_first_that_does_not(gpu, bits, fits, refused):
    from amatsukaze_amd import AmtError, Resizer
    (cpw, K, spans), (cpwC, KC, spansC) = cpw_of(fits, 2, bits)
    assert (cpw, K, spans) == (64, fits, (2000,)) and (cpwC, KC, spansC) == (64, fits // 2, (1000,))      # K = S; chroma D = 1
    assert cpw_of(refused, 2, bits)[0][0] == 0 and cpw_of(refused, 2, bits)[1][0] == 64                    # luma alone is refused
    with pytest.raises(AmtError, match="does not fit a wave's staging region"):                          # (a create launches nothing)
        Resizer(gpu[0], (refused, 8), (2, 8), bits)
    for layouts in (aligned_layouts, narrow_layouts):
        case(gpu, "%d -> 2" % fits, 2, (fits, 8), (2, 8), bits, layouts)


# ---- 4. several chunks per row in the vertical 16-byte form ----
def test_three_and_two_chunks_per_row_at_8_bits(gpu):
    assert chunks_of(2080, 8) == (130, 3) and chunks_of(1040, 8) == (65, 2)
    (cpw, K, spans), _ = cpw_of(2176, 2080, 8)
    assert (cpw, K, len(spans)) == (64, 9, 33) and 2080 == 32 * 64 + 32 and R.program(12, 8)[0] == 12 and R.program(6, 4)[0] == 6
    assert vec_form(aligned_layouts, 2176, 12, 2080, 8, 8)
    case(gpu, "2176x12 -> 2080x8", 2, (2176, 12), (2080, 8), 8, aligned_layouts)


def test_a_second_chunk_with_one_live_lane_at_10_bits(gpu):
    assert chunks_of(1040, 10) == (130, 3) and chunks_of(520, 10) == (65, 2)    # chroma: lane 0 of the second chunk, 63 lanes past the row
    assert vec_form(aligned_layouts, 1088, 12, 1040, 8, 10)
    case(gpu, "1088x12 -> 1040x8", 2, (1088, 12), (1040, 8), 10, aligned_layouts)


def test_a_partial_lane_in_the_second_chunk(gpu):
    lanes, chunks = chunks_of(1046, 8)
    assert (lanes, chunks) == (66, 2) and 1046 - 65 * 16 == 6           # lane 1 of the second chunk holds 6 containers
    assert chunks_of(523, 8) == (33, 1) and 523 % 16 == 11              # ... and chroma has its partial lane in the first
    assert vec_form(aligned_layouts, 1094, 12, 1046, 8, 8)
    case(gpu, "1094x12 -> 1046x8", 2, (1094, 12), (1046, 8), 8, aligned_layouts)


# ---- 5. windows the unrolled loops do not divide ----
@BOTH
@pytest.mark.parametrize("bits", [8, 10])
def test_windows_of_22_on_both_axes(gpu, bits, layouts):
    assert R.program(100, 38)[0] == 22 and R.program(50, 19)[0] == 22 and 22 % 4 == 2 and 22 > 16
    case(gpu, "100x100 -> 38x38", 2, (100, 100), (38, 38), bits, layouts)


def test_explicit_taps_widen_the_windows(gpu):
    Ks = [R.program(S, D, "blackman", 8)[0] for S, D in ((48, 32), (36, 24), (24, 16), (18, 12))]
    assert Ks == [24, 24, 24, 18] and R.program(48, 32)[0] == 12         # chroma rows: K = S = 18
    planes, default = noise_case(2, 48, 36, 32, 24, 10)
    want = R.resize_clip(planes, 32, 24, 10, "blackman", 8)
    assert not np.array_equal(want[0], default[0])
    for layouts in (aligned_layouts, narrow_layouts):
        run_resize(gpu, ("taps 8", layouts.__name__), planes, 10, (32, 24), layouts, want, taps=8)     # (compares the device's programs too)


# ---- 6. one object, several calls ----
def test_one_resizer_grows_its_intermediate_and_switches_forms(gpu):
    from amatsukaze_amd import Resizer
    ctx, torch = gpu
    bits, src, dst = 10, (48, 36), (32, 24)
    planes, want = noise_case(3, *src, *dst, bits)
    one = 64 * 36 + 2 * 32 * 18                                         # one frame's intermediate (test_gpu_resize.py)
    rz = Resizer(ctx, src, dst, bits, max_scratch_bytes=4 * one - 1)    # three frames a round: a call of one frame allocates one
    assert vec_form(aligned_layouts, *src, *dst, bits) and not vec_form(narrow_layouts, *src, *dst, bits)

    def call(what, n, layouts):
        sl, dl = layouts(*src, *dst, bits)
        src_host = Buf(n, *src, bits, **sl).put(tuple(p[:n] for p in planes))
        dst_host = sentinel_buf(n, *dst, bits, dl)
        s, s_flat = upload(gpu, src_host)
        d, d_flat = upload(gpu, dst_host)
        assert rz.run(s, d) == n
        torch.cuda.synchronize()
        got = download(dst_host, d_flat)
        check_against(what, dst_host, got, tuple(w[:n] for w in want))
        for g, a in zip(download(src_host, s_flat), src_host.flat):
            assert np.array_equal(g, a), (what, "the source changed")
        return got

    try:
        call("one frame, 16-byte form", 1, aligned_layouts)
        second = call("three frames: the intermediate grows", 3, aligned_layouts)
        call("three frames, container form", 3, narrow_layouts)
        last = call("three frames, 16-byte form again", 3, aligned_layouts)
    finally:
        rz.close()
    for a, b in zip(second, last):
        assert np.array_equal(a, b)


# ---- 7. one side aligned ----
@pytest.mark.parametrize("layouts, sides", [(aligned_to_narrow, (True, False)), (narrow_to_aligned, (False, True))], ids=["aligned to narrow", "narrow to aligned"])
@pytest.mark.parametrize("bits", [8, 10])
def test_one_unaligned_side_takes_both_stages_to_the_container_form(gpu, bits, layouts, sides):
    assert rows_on_16_bytes(layouts, 272, 48, 182, 34, bits) == sides and not vec_form(layouts, 272, 48, 182, 34, bits)
    assert R.program(272, 182)[0] == 12
    case(gpu, "272x48 -> 182x34", 2, (272, 48), (182, 34), bits, layouts)
