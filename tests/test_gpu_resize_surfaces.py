"""The resize on decoder surfaces on the GPU (amtgpu_resize_run_surfaces, Resizer.run on NV12 / P010 / P012 / P016 / interleaved LSB /
planar MSB pairs in kind) against its composed numpy restatement (tests/resize_surfaces_ref.py): every container of
the destination buffers, the containers behind the rows and in front of, between and behind the frames included; sources unchanged;
16-byte and container-by-container forms; every K form; pair runs with tails; per-component edge folding; low bits in and out;
components that must not mix; rounds; the staging region at pair size; planar LSB pairs through the new entry point; the chain into the
temporal NR; and every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import resize_ref as R
import resize_surfaces_ref as RS
import temporal_nr_ref as TR
import temporal_nr_surfaces_ref as TS
from test_gpu_temporal_nr_surfaces import (KINDS, PLANAR, SBuf, aligned_layouts, assert_unchanged, check_against, download, half_aligned_layouts,
                                           narrow_layouts, packed, sentinel_buf, upload)

pytestmark = pytest.mark.gpu

LAYOUTS = {"aligned": aligned_layouts, "narrow": narrow_layouts, "half": half_aligned_layouts}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    ctx = Context(0)
    yield ctx, torch
    ctx.close()


@functools.lru_cache(maxsize=None)
def noise_case(n, sw, sh, dw, dh, name, kernel="blackman", seed=0):
    """(the surface's tight planes of seeded noise over the depth's whole range, random non-zero low bits where the kind has any; the
    expected tight planes); computed once, read-only"""
    kind = KINDS.get(name) or PLANAR[int(name)]
    bits, il, msb = kind
    samples = R.make_clip(n, sw, sh, bits, np.random.default_rng(sw * 131 + sh * 7 + dw * 3 + dh + bits + seed))
    planes = packed(samples, kind, sw + dh + seed)
    want = RS.resize_surfaces(planes, dw, dh, bits, il, msb, kernel)
    for a in (*planes, *want):
        a.setflags(write=False)
    return planes, want


def place(gpu, kind, planes, dst_size, layouts):
    """(source host buffers, device surfaces, flat tensors, and the same three of a sentinel destination)"""
    n, sh, sw = planes[0].shape
    dw, dh = dst_size
    src_host = SBuf(n, sw, sh, kind, **layouts(sw, sh, kind)[0]).put(planes)
    dst_host = sentinel_buf(n, dw, dh, kind, layouts(dw, dh, kind)[1])
    return (src_host, *upload(gpu, src_host)), (dst_host, *upload(gpu, dst_host))


def run_resize(gpu, what, kind, planes, dst_size, layouts, want, kernel="blackman", max_scratch_bytes=None):
    """resizes the whole clip in one call and compares every destination container; the sources must stay as they were and no output
    container may hold a low bit.  Returns the destination's flat buffers as they came back"""
    from amatsukaze_amd import Resizer
    ctx, torch = gpu
    bits, il, msb = kind
    n, sh, sw = planes[0].shape
    (src_host, src, src_flat), (dst_host, dst, dst_flat) = place(gpu, kind, planes, dst_size, layouts)
    assert (src.V is None) == il
    rz = Resizer(ctx, (sw, sh), dst_size, bits, kernel=kernel, max_scratch_bytes=max_scratch_bytes)
    try:
        assert rz.run(src, dst) == n
    finally:
        rz.close()
    torch.cuda.synchronize()
    got = download(dst_host, dst_flat)
    check_against(what, dst_host, got, want)
    assert_unchanged(what, src_host, src_flat)
    low = (1 << TS.shift_of(bits, msb)) - 1
    for k in range(len(want)):
        assert not np.any(dst_host.view(k, got[k]) & low), (what, "low bits in the output")
    return got


# ---- shapes ----
@pytest.mark.parametrize("layouts", ["aligned", "narrow", "half"])
@pytest.mark.parametrize("name", list(KINDS))
def test_three_to_two(gpu, name, layouts):
    # 48x36 -> 32x24: K 12 in luma and chroma.  aligned: the 16-byte forms; narrow: bases one container off, odd pitches; half: the
    # source's UV rows 8 bytes off a 16-byte boundary, which the lane rule must send to the container form
    assert R.program(48, 32)[0] == 12 and R.program(24, 16)[0] == 12
    planes, want = noise_case(2, 48, 36, 32, 24, name)
    run_resize(gpu, ("3:2", name, layouts), KINDS[name], planes, (32, 24), LAYOUTS[layouts], want)


@pytest.mark.parametrize("layouts", ["aligned", "narrow"])
@pytest.mark.parametrize("name", ["nv12", "p010"])
def test_an_irregular_ratio_with_three_pair_runs_and_a_tail(gpu, name, layouts):
    # 272x48 -> 182x34: a chroma row has 91 columns -- pair runs of 32, 32 and 27 --, a luma row three runs, the last of 54
    es = 1 if name == "nv12" else 2
    assert RS.pair_columns_per_wave(136, 91, es)[0] == 32 and 91 - 2 * 32 == 27 and R.columns_per_wave(272, 182, es)[0] == 64 and 182 - 2 * 64 == 54
    planes, want = noise_case(2, 272, 48, 182, 34, name)
    run_resize(gpu, ("272 -> 182", name, layouts), KINDS[name], planes, (182, 34), LAYOUTS[layouts], want)


@pytest.mark.parametrize("name", ["nv12", "p010"])
def test_upscaling_has_coefficients_above_one(gpu, name):
    K, _, Cf = R.program(32, 50)
    assert K == 8 and int(Cf.max()) == 17723 and int(Cf.min()) < 0
    planes, want = noise_case(2, 32, 24, 50, 40, name)
    run_resize(gpu, ("32x24 -> 50x40", name), KINDS[name], planes, (50, 40), aligned_layouts, want)


@pytest.mark.parametrize("layouts", ["aligned", "narrow"])
@pytest.mark.parametrize("name", list(KINDS))
def test_windows_as_wide_as_the_plane_fold_per_component(gpu, name, layouts):
    # 16x8 -> 8x4: K = S = 16 in luma rows; in chroma 8 -> 4 folds K0 = 16 into K = S = 8, and 4 -> 2 into 4: the clamp at the row's
    # ends is per component -- an interleaved row's last U is its last container but one
    assert R.program(16, 8)[0] == 16 and R.program(8, 4)[0] == 8 and R.program(4, 2)[0] == 4
    planes, want = noise_case(3, 16, 8, 8, 4, name)
    run_resize(gpu, ("16x8 -> 8x4", name, layouts), KINDS[name], planes, (8, 4), LAYOUTS[layouts], want)


@pytest.mark.parametrize("name", ["nv12", "p010"])
def test_the_table_walk_takes_windows_above_16_taps(gpu, name):
    # 160 -> 32 has K 40; chroma 80 -> 16 too, its taps two containers apart
    assert R.program(160, 32)[0] == 40 and R.program(80, 16)[0] == 40
    planes, want = noise_case(2, 160, 24, 32, 16, name)
    run_resize(gpu, ("160x24 -> 32x16", name), KINDS[name], planes, (32, 16), aligned_layouts, want)


@pytest.mark.parametrize("layouts", ["aligned", "narrow"])
@pytest.mark.parametrize("name", list(KINDS))
def test_equal_sizes_copy_the_samples_and_drop_the_low_bits(gpu, name, layouts):
    kind = KINDS[name]
    bits, il, msb = kind
    s = TS.shift_of(bits, msb)
    planes, want = noise_case(2, 64, 32, 64, 32, name)
    for p, w in zip(planes, want):
        assert np.array_equal(p >> s, w >> s) and not np.any(w & ((1 << s) - 1))      # the reference itself: a single 16384 per row
        assert np.array_equal(p, w) == (s == 0)                                       # at nv12 and il10 dst is src; elsewhere the low bits go
    run_resize(gpu, ("64x32 -> 64x32", name, layouts), kind, planes, (64, 32), LAYOUTS[layouts], want)


@pytest.mark.parametrize("kernel, K", [("lanczos", 9), ("bilinear", 3)])
def test_the_other_kernels(gpu, kernel, K):
    assert R.program(48, 32, kernel)[0] == K
    planes, want = noise_case(2, 48, 36, 32, 24, "p010", kernel)
    assert not np.array_equal(want[1], noise_case(2, 48, 36, 32, 24, "p010")[1][1])
    run_resize(gpu, kernel, KINDS["p010"], planes, (32, 24), aligned_layouts, want, kernel=kernel)


# ---- low bits ----
@pytest.mark.parametrize("layouts", ["aligned", "narrow"])
@pytest.mark.parametrize("name", ["p010", "pmsb10"])
def test_the_sources_low_bits_change_no_byte(gpu, name, layouts):
    kind = KINDS[name]
    bits, il, msb = kind
    s = TS.shift_of(bits, msb)
    samples = R.make_clip(2, 48, 36, bits, np.random.default_rng(bits))
    one, two = packed(samples, kind, 1), packed(samples, kind, 2)
    assert all(np.all(a & ((1 << s) - 1)) and np.all(b & ((1 << s) - 1)) and np.mean(a != b) > 0.5 for a, b in zip(one, two))
    assert all(np.array_equal(a >> s, b >> s) for a, b in zip(one, two))
    want = RS.resize_surfaces(one, 32, 24, bits, il, msb)
    g1 = run_resize(gpu, (name, "low bits 1"), kind, one, (32, 24), LAYOUTS[layouts], want)
    g2 = run_resize(gpu, (name, "low bits 2"), kind, two, (32, 24), LAYOUTS[layouts], want)
    for a, b in zip(g1, g2):
        assert np.array_equal(a, b)


# ---- components do not mix ----
@pytest.mark.parametrize("layouts", ["aligned", "narrow"])
@pytest.mark.parametrize("name", ["nv12", "p010"])
def test_constant_components_stay_constant(gpu, name, layouts):
    # U constant 0 beside V constant maxv, and the reverse: sum C = 16384, so one tap taken from the other component shows
    kind = KINDS[name]
    bits, il, msb = kind
    maxv = (1 << bits) - 1
    dt = np.uint8 if bits <= 8 else np.uint16
    for u, v in ((0, maxv), (maxv, 0)):
        samples = (R.make_clip(2, 48, 36, bits, np.random.default_rng(u))[0], np.full((2, 18, 24), u, dt), np.full((2, 18, 24), v, dt))
        want = RS.resize_surfaces(packed(samples, kind, 3), 32, 24, bits, il, msb)
        wY, wU, wV = TS.unpack(want, bits, il, msb)
        assert np.all(wU == u) and np.all(wV == v)
        run_resize(gpu, ("constants", name, u, v), kind, packed(samples, kind, 3), (32, 24), LAYOUTS[layouts], want)


@pytest.mark.parametrize("layouts", ["aligned", "narrow"])
def test_step_edges_at_different_columns_of_u_and_v_reach_both_clamps(gpu, layouts):
    kind = KINDS["p016"]
    bits, maxv = 16, 65535
    U = np.zeros((2, 18, 24), np.uint16); V = np.zeros((2, 18, 24), np.uint16)
    U[0, :, 12:] = maxv; U[1, :, :9] = maxv
    V[0, :, 7:] = maxv; V[1, :, :17] = maxv
    samples = (R.make_clip(2, 48, 36, bits, np.random.default_rng(16))[0], U, V)
    # the unclamped sums of the stage that crosses the edges leave 0 .. maxv on both sides, in each component
    K, start, Cf = R.program(24, 16)
    for comp in (U, V):
        for f in range(2):
            acc = (comp[f, 0, :].astype(np.int64)[start[:, None] + np.arange(K)[None, :]] * Cf).sum(axis=1)
            assert acc.min() < 0 and acc.max() > maxv * 16384 and acc.max() + 8192 < 2 ** 31
    planes = packed(samples, kind, 0)
    want = RS.resize_surfaces(planes, 32, 24, bits, True, True)
    _, wU, wV = TS.unpack(want, bits, True, True)
    assert int(wU.min()) == int(wV.min()) == 0 and int(wU.max()) == int(wV.max()) == maxv and not np.array_equal(wU, wV)
    run_resize(gpu, "step edges", kind, planes, (32, 24), LAYOUTS[layouts], want)


# ---- rounds ----
def test_rounds_give_the_bytes_of_the_default(gpu):
    planes, want = noise_case(3, 48, 36, 32, 24, "p010")
    # one frame's intermediate, as the planar object's: rows of the destination's width rounded up to 16 bytes, the source's height of
    # them, for three planes -- the interleaved UV plane fits the two chroma planes' room
    one = 64 * 36 + 2 * 32 * 18
    whole = run_resize(gpu, "default scratch", KINDS["p010"], planes, (32, 24), aligned_layouts, want)
    rounds = run_resize(gpu, "one frame per round", KINDS["p010"], planes, (32, 24), aligned_layouts, want, max_scratch_bytes=one)
    pairs = run_resize(gpu, "two frames, then one", KINDS["p010"], planes, (32, 24), aligned_layouts, want, max_scratch_bytes=2 * one + 17)
    for a, b, c in zip(whole, rounds, pairs):
        assert np.array_equal(a, b) and np.array_equal(a, c)


# ---- the staging region at pair size ----
def pair_limits():
    """(the widest source whose interleaved chroma window still fits at 16 bits into 16 output columns, the first that does not), from
    the ported rule: chroma S / 2 -> 8 has K = S / 2 pairs of 4 bytes"""
    fits = [sw for sw in range(800, 1400, 2) if RS.pair_columns_per_wave(sw // 2, 8, 2)[0]]
    return max(fits), max(fits) + 2


def test_the_widest_interleaved_chroma_window_that_fits(gpu):
    sw, _ = pair_limits()
    cpw, K, spans = RS.pair_columns_per_wave(sw // 2, 8, 2)
    assert cpw >= 1 and max(spans) + RS.PAIR_SLACK <= RS.REGION_BYTES < max(spans) + 4 + RS.PAIR_SLACK and K > 16, (sw, cpw, K, spans)
    planes, want = noise_case(2, sw, 8, 16, 8, "p010")
    run_resize(gpu, ("widest", sw), KINDS["p010"], planes, (16, 8), aligned_layouts, want)


def test_the_first_window_that_does_not_fit_is_refused_on_interleaved_surfaces_alone(gpu):
    from amatsukaze_amd import AmtError, Resizer
    ctx, torch = gpu
    _, sw = pair_limits()
    assert RS.pair_columns_per_wave(sw // 2, 8, 2)[0] == 0 and R.columns_per_wave(sw // 2, 8, 2)[0] >= 1 and R.columns_per_wave(sw, 16, 2)[0] >= 1
    planes, _ = noise_case(2, sw, 8, 16, 8, "p010")
    (src_host, src, src_flat), (dst_host, dst, dst_flat) = place(gpu, KINDS["p010"], planes, (16, 8), aligned_layouts)
    rz = Resizer(ctx, (sw, 8), (16, 8), 10)                                      # the object is made: planar surfaces can run
    try:
        with pytest.raises(AmtError, match="does not fit a wave's staging region"):
            rz.run(src, dst)
    finally:
        rz.close()
    torch.cuda.synchronize()
    assert_unchanged("refused", dst_host, dst_flat)                              # still the sentinel, everywhere
    assert_unchanged("refused", src_host, src_flat)
    for name in ("pmsb10", "10"):
        kind = KINDS.get(name) or PLANAR[10]
        planes, want = noise_case(2, sw, 8, 16, 8, name)
        run_resize(gpu, ("planar at the refused size", name), kind, planes, (16, 8), aligned_layouts, want)


def test_pair_runs_halve_while_luma_runs_stay_at_64(gpu):
    # luma 64 columns of a run read 72 r samples of 2 bytes at ratio r, a pair run of 32 reads 40 r pairs of 4 bytes: between them lies r = 13
    # (192 output columns: a row has runs in its middle, whose windows no edge clamps)
    sw = next(w for w in range(192 * 4, 192 * 16, 192) if R.columns_per_wave(w, 192, 2)[0] == 64 and RS.pair_columns_per_wave(w // 2, 96, 2)[0] < 32)
    cpw = RS.pair_columns_per_wave(sw // 2, 96, 2)[0]
    assert 1 <= cpw <= 16, (sw, cpw)
    planes, want = noise_case(2, sw, 8, 192, 8, "p010")
    run_resize(gpu, ("pair runs of", cpw, "at", sw), KINDS["p010"], planes, (192, 8), aligned_layouts, want)


# ---- planar LSB pairs through the new entry point ----
@pytest.mark.parametrize("layouts", ["aligned", "narrow"])
@pytest.mark.parametrize("bits", [8, 10])
def test_a_planar_lsb_pair_through_the_new_entry_point_is_resize_run(gpu, bits, layouts):
    from amatsukaze_amd import Resizer
    ctx, torch = gpu
    kind = PLANAR[bits]
    planes, want = noise_case(2, 48, 36, 32, 24, str(bits))
    (src_host, src, src_flat), (dst_host, old, old_flat) = place(gpu, kind, planes, (32, 24), LAYOUTS[layouts])
    new, new_flat = upload(gpu, dst_host)
    rz = Resizer(ctx, (48, 36), (32, 24), bits)
    try:
        s, a, b = src.ref(), old.ref(), new.ref()
        assert not s.interleaved and not s.msb_aligned
        assert ctx.lib.amtgpu_resize_run(rz.h, C.byref(s), C.byref(a), 2) == 1
        assert ctx.lib.amtgpu_resize_run_surfaces(rz.h, C.byref(s), C.byref(b), 2) == 1, ctx.lib.amtgpu_last_error(ctx.h)
    finally:
        rz.close()
    torch.cuda.synchronize()
    one, two = download(dst_host, old_flat), download(dst_host, new_flat)
    for x, y in zip(one, two):
        assert np.array_equal(x, y)
    check_against(("planar", bits), dst_host, two, want)
    assert_unchanged(("planar", bits), src_host, src_flat)


# ---- the chain: resize, then the temporal NR, both in kind ----
def test_the_resize_feeds_the_temporal_nr_in_kind(gpu):
    from amatsukaze_amd import Resizer, temporal_nr
    ctx, torch = gpu
    kind = KINDS["p010"]
    n, d, thr = 5, 1, 3
    samples = TR.make_clip(n, 48, 36, 10, thr, np.random.default_rng(48))
    planes = packed(samples[:3], kind, 5)
    mid_want = RS.resize_surfaces(planes, 32, 24, 10, True, True)
    want, _ = TS.filter_surfaces(mid_want, d, thr, 10, True, True)
    assert any(not np.array_equal(a, b) for a, b in zip(mid_want, want))         # the NR does something to the resized clip
    (src_host, src, src_flat), (mid_host, mid, mid_flat) = place(gpu, kind, planes, (32, 24), aligned_layouts)
    out_host = sentinel_buf(n, 32, 24, kind, aligned_layouts(32, 24, kind)[1])
    out, out_flat = upload(gpu, out_host)
    rz = Resizer(ctx, (48, 36), (32, 24), 10)
    try:
        assert rz.run(src, mid) == n
    finally:
        rz.close()
    assert temporal_nr(ctx, mid, out, distance=d, threshold=thr) == (0, n)       # the resize's output is the NR's source, as it lies
    torch.cuda.synchronize()
    check_against("resized", mid_host, download(mid_host, mid_flat), mid_want)
    check_against("resized and filtered", out_host, download(out_host, out_flat), want)
    assert_unchanged("chain", src_host, src_flat)


# ---- refusals ----
def test_refusals_launch_nothing(gpu):
    from amatsukaze_amd import AmtError, Resizer, binding
    ctx, torch = gpu
    N, sw, sh, dw, dh = 3, 48, 36, 32, 24
    clips = {}

    def pair(name):
        kind = KINDS.get(name) or PLANAR[int(name)]
        planes, _ = noise_case(N, sw, sh, dw, dh, name)
        clips[name] = place(gpu, kind, planes, (dw, dh), aligned_layouts)
        return clips[name][0][1].ref(), clips[name][1][1].ref()

    def changed(desc, **kw):
        c = binding.Surfaces()
        C.memmove(C.byref(c), C.byref(desc), C.sizeof(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    nv_s, nv_d = pair("nv12")
    pl8_s, pl8_d = pair("8")
    p10_s, p10_d = pair("p010")
    il_s, il_d = pair("il10")
    pm_s, pm_d = pair("pmsb10")
    pl10_s, pl10_d = pair("10")
    rz8, rz10 = Resizer(ctx, (sw, sh), (dw, dh), 8), Resizer(ctx, (sw, sh), (dw, dh), 10)
    assert nv_s.interleaved and nv_s.pitchUV >= sw and p10_d.pitchUV >= dw

    def call(r_, s_, t_, n):
        r = ctx.lib.amtgpu_resize_run_surfaces(r_.h, C.byref(s_), C.byref(t_), n)
        return r, ctx.lib.amtgpu_last_error(ctx.h).decode(errors="replace")

    last_uv_byte = nv_s.U + nv_s.strideUV * (N - 1) + (sh // 2 - 1) * nv_s.pitchUV + sw - 1        # of the source's UV rows of `width` containers
    cases = {
        "NV12 into planes": (rz8, nv_s, pl8_d, N, "not in kind"),
        "planes into NV12": (rz8, pl8_s, nv_d, N, "converts no layouts"),
        "P010 into planar MSB": (rz10, p10_s, pm_d, N, "not in kind"),
        "planar MSB into P010": (rz10, pm_s, p10_d, N, "not in kind"),
        "P010 into interleaved LSB": (rz10, p10_s, il_d, N, "not in kind"),
        "interleaved LSB into P010": (rz10, il_s, p10_d, N, "not in kind"),
        "planar MSB into planar LSB": (rz10, pm_s, pl10_d, N, "converts no layouts"),
        "planar LSB into planar MSB": (rz10, pl10_s, pm_d, N, "converts no layouts"),
        "P010 on the 8-bit object": (rz8, p10_s, p10_d, N, "source: 10 bits, the resizer was created for 8"),
        "a destination that says P012": (rz10, p10_s, changed(p10_d, bits=12), N, "destination: 12 bits, the resizer was created for 10"),
        "MSB-aligned at 8 bits": (rz8, changed(nv_s, msb_aligned=1), changed(nv_d, msb_aligned=1), N, "MSB-aligned surfaces are 16-bit containers"),
        "interleaved source pitchUV below width": (rz8, changed(nv_s, pitchUV=sw - 2), nv_d, N, "source: pitch smaller than the row"),
        "interleaved destination pitchUV below width": (rz10, p10_s, changed(p10_d, pitchUV=dw - 1), N, "destination: pitch smaller than the row"),
        "source luma pitch below the row": (rz10, changed(p10_s, pitchY=sw - 2), p10_d, N, "source: pitch smaller than the row"),
        "negative source stride": (rz10, changed(p10_s, strideY=-p10_s.strideY), p10_d, N, "source: negative frame stride"),
        "negative destination chroma stride": (rz8, nv_s, changed(nv_d, strideUV=-nv_d.strideUV), N, "destination: negative frame stride"),
        "overlapping destination UV frames": (rz8, nv_s, changed(nv_d, strideUV=(dh // 2 - 1) * nv_d.pitchUV + dw - 1), 2, "destination frames overlap each other"),
        "overlapping destination luma frames": (rz10, p10_s, changed(p10_d, strideY=((dh - 1) * p10_d.pitchY + dw - 1) * 2), 2, "destination frames overlap each other"),
        "destination is the source": (rz10, p10_s, changed(p10_s), N, "overlaps the source's"),
        "destination UV inside the source's luma": (rz8, nv_s, changed(nv_d, U=nv_s.Y), 1, "overlaps the source's"),
        "destination luma on the last byte of the source's UV rows": (rz8, nv_s, changed(nv_d, Y=last_uv_byte), N, "overlaps the source's"),
        "null Y plane": (rz10, changed(p10_s, Y=None), p10_d, N, "null surface plane"),
        "null UV plane": (rz10, p10_s, changed(p10_d, U=None), N, "null surface plane"),
        "null V plane of planar MSB": (rz10, changed(pm_s, V=None), pm_d, N, "null surface plane"),
        "negative frame count": (rz10, p10_s, p10_d, -1, "negative frame count"),
    }
    for what, (r_, s_, t_, n, words) in cases.items():
        r, msg = call(r_, s_, t_, n)
        assert r == 0 and words in msg and "[Resize]" in msg, (what, msg)
    assert call(rz10, p10_s, p10_d, 0)[0] == 1                                                         # nothing to resize: 1
    with pytest.raises(AmtError, match="not in kind"):
        rz8.run(clips["nv12"][0][1], clips["8"][1][1])                                                 # a mixed pair from Python
    torch.cuda.synchronize()
    for name, both in clips.items():
        for host, _, flat_t in both:
            assert_unchanged(name, host, flat_t)                     # sources as they were, destinations still the sentinel everywhere
    # ... and the same objects and buffers do the work once nothing is wrong: the first two frames
    for rz, name, s_, t_ in ((rz8, "nv12", nv_s, nv_d), (rz10, "p010", p10_s, p10_d)):
        r, msg = call(rz, s_, t_, 2)
        assert r == 1, msg
        torch.cuda.synchronize()
        dst_host, _, dst_flat = clips[name][1]
        check_against(("two frames", name), dst_host, download(dst_host, dst_flat), tuple(w[:2] for w in noise_case(N, sw, sh, dw, dh, name)[1]))
    rz8.close()
    rz10.close()
