"""The deband on decoder surfaces on the GPU (amtgpu_deband_run_surfaces on NV12 / P010 / P012 / P016 / interleaved LSB / planar MSB
pairs in kind; DESIGN.md section 6f, "surfaces in kind") against its composed numpy restatement (tests/deband_surfaces_ref.py): every
container of the destination buffers, the bytes behind the rows and in front of, between and behind the frames included, on all eight
kernel forms; the planar test's sizes, radii, samples and blur_first; planted tables that reach the outermost halo of the interleaved
UV plane; U and V that must not mix; low bits in and out; sums of four 65 535s; the planar route on the same samples; planar LSB pairs
through the new entry point; a clip cut into calls; the chain resize -> temporal NR -> deband on P010; and every refusal."""
import ctypes as C

import numpy as np
import pytest

import deband_ref as R
import deband_surfaces_ref as DS
import temporal_nr_surfaces_ref as TS
from test_gpu_deband import DIRECTIONS, MODES, clip
from test_gpu_temporal_nr_surfaces import (KINDS, PLANAR, SBuf, aligned_layouts, assert_unchanged, check_against, cut, download, half_aligned_layouts,
                                           narrow_layouts, packed, sentinel_buf, upload)

pytestmark = pytest.mark.gpu

SIZES = [(2, 2), (8, 6), (130, 98), (290, 198)]                        # the planar test's: TW + 2, TH + 2; 2 TW + 34, 2 TH + 6
LAYOUTS = {"aligned": aligned_layouts, "narrow": narrow_layouts, "half": half_aligned_layouts}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    ctx = Context(0)
    yield ctx, torch
    ctx.close()


def samples_of(w, h, bits, what, n=2):
    """(Y, U, V) samples of test_gpu_deband.clip at the kind's depth"""
    return clip(w, h, (bits, bits), what, n)


def run_case(gpu, what, kind, planes, layouts, want, offsets=None, **params):
    """one call over the whole clip of packed surface planes: every destination container against `want`, the sources unchanged, zero
    low bits in the output.  offsets: the three COMPONENT planes' (dx, dy).  Returns the destination's frames as tight planes"""
    from amatsukaze_amd import Debander
    ctx, torch = gpu
    bits, interleaved, msb = kind
    n, h, w = planes[0].shape
    sl, dl = layouts(w, h, kind)
    src_host = SBuf(n, w, h, kind, **sl).put(planes)
    dst_host = sentinel_buf(n, w, h, kind, dl)
    src, src_flat = upload(gpu, src_host)
    dst, dst_flat = upload(gpu, dst_host)
    assert (src.V is None) == interleaved
    db = Debander(ctx, (w, h), bits, **params)
    if offsets is not None:
        for p, (dx, dy) in enumerate(offsets):
            db.set_offsets(p, dx, dy)
    assert db.run(src, dst) == n
    db.close()
    torch.cuda.synchronize()
    got = download(dst_host, dst_flat)
    check_against(what, dst_host, got, want)
    assert_unchanged(what, src_host, src_flat)
    low = (1 << TS.shift_of(bits, msb)) - 1
    frames = tuple(np.array(dst_host.view(k, got[k])) for k in range(len(want)))
    for f in frames:
        assert not np.any(f & low), (what, "low bits in the output")
    return frames


# ---- every kind, every layout, at the planar test's sizes ----
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["nv12", "p010", "p012", "p016", "il10", "pmsb10"])
def test_every_kind_and_layout_at_the_planar_tests_sizes(gpu, name, size, layout):
    kind = KINDS[name]
    bits, interleaved, msb = kind
    w, h = size
    samples = samples_of(w, h, bits, "soft")
    planes = packed(samples, kind, w + h)
    want = DS.deband_surfaces(planes, bits, interleaved, msb)           # the defaults: 25, 1, 2, true, seed 0
    if w >= 128:
        changed = float(np.mean(TS.unpack(want, bits, interleaved, msb)[0] != samples[0]))
        assert 0.02 < changed < 0.98, changed                           # the threshold keeps some pixels and filters others
    run_case(gpu, (name, size, layout), kind, planes, LAYOUTS[layout], want)


# ---- every mode ----
@pytest.mark.parametrize("radius", [1, 25, 31])
@pytest.mark.parametrize("layout", ["aligned", "narrow"])
@pytest.mark.parametrize("name", ["nv12", "p010"])
def test_every_radius_sample_and_blur_first(gpu, name, layout, radius):
    kind = KINDS[name]
    bits, interleaved, msb = kind
    w, h = SIZES[3]
    for what, threshold in (("random", 32767), ("soft", 2)):
        planes = packed(samples_of(w, h, bits, what), kind, radius)
        outputs = {}
        for sample, bf in MODES:
            want = DS.deband_surfaces(planes, bits, interleaved, msb, radius, threshold, sample, bf, seed=radius)
            outputs[(sample, bf)] = want
            run_case(gpu, (name, layout, radius, sample, bf, what), kind, planes, LAYOUTS[layout], want,
                     radius=radius, threshold=threshold, sample=sample, blur_first=bf, seed=radius)
        if what == "soft":
            for sample in (1, 2):                                       # the two blur_first settings give other bytes
                assert not np.array_equal(outputs[(sample, True)][0], outputs[(sample, False)][0]), (radius, sample)


# ---- planted tables: every pixel's references on the rim of what it may reach ----
@pytest.mark.parametrize("radius", [25, 31])
@pytest.mark.parametrize("layout", ["aligned", "narrow"])
@pytest.mark.parametrize("size", SIZES[2:], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["nv12", "p016"])
def test_planted_tables_read_the_outermost_halo(gpu, name, size, layout, radius):
    kind = KINDS[name]
    bits, interleaved, msb = kind
    w, h = size
    planes = packed(samples_of(w, h, bits, "random"), kind, radius)
    for sx, sy in DIRECTIONS:
        offsets = []
        for p in range(3):
            lim = R.lim_map(*R.plane_size(p, w, h), R.plane_radius(p, radius))
            offsets.append(((sx * lim).astype(np.int8), (sy * lim).astype(np.int8)))
        # an interior chroma pixel's references are radius >> 1 components away: 2 * (radius >> 1) containers of the UV row, and
        # radius >> 1 rows; the first and last row and column of every tile read the outermost row and column of its halo
        assert int(np.abs(offsets[0][0]).max() + np.abs(offsets[0][1]).max()) >= radius
        assert int(np.abs(offsets[1][0]).max() + np.abs(offsets[1][1]).max()) >= radius >> 1 and 2 * (radius >> 1) == (24, 30)[radius == 31]
        want = DS.deband_surfaces(planes, bits, interleaved, msb, radius, 32767, 2, True, offsets=offsets)
        run_case(gpu, (name, size, layout, radius, sx, sy), kind, planes, LAYOUTS[layout], want, offsets=offsets,
                 radius=radius, threshold=32767, sample=2, blur_first=True)


# ---- U and V do not mix ----
@pytest.mark.parametrize("layout", ["aligned", "narrow"])
@pytest.mark.parametrize("name", ["nv12", "p010"])
def test_components_do_not_mix(gpu, name, layout):
    kind = KINDS[name]
    bits, interleaved, msb = kind
    w, h = SIZES[2]
    A, B = 3 << (bits - 8), 201 << (bits - 8)
    Y = samples_of(w, h, bits, "random")[0]
    dt = Y.dtype
    # constants: whatever the tables say, a U reference that were a V container would move the average off A
    const = (Y, np.full((2, h // 2, w // 2), A, dt), np.full((2, h // 2, w // 2), B, dt))
    planes = packed(const, kind, 5)
    want = DS.deband_surfaces(planes, bits, interleaved, msb, 25, 32767, 2, True, seed=11)
    got = run_case(gpu, (name, layout, "constants"), kind, planes, LAYOUTS[layout], want, radius=25, threshold=32767, sample=2, blur_first=True, seed=11)
    _, U, V = TS.unpack(got, bits, interleaved, msb)
    assert np.all(U == A) and np.all(V == B)
    # U's table sends every pixel lim to the right, V's is zeros: V out is V in, U is the restatement's
    samples = samples_of(w, h, bits, "random")
    planes = packed(samples, kind, 6)
    offsets = [R.table(0, w, h, 25, 11)]
    lim = R.lim_map(w // 2, h // 2, 12)
    zeros = np.zeros_like(lim, np.int8)
    offsets += [(lim.astype(np.int8), zeros), (zeros, zeros)]
    want = DS.deband_surfaces(planes, bits, interleaved, msb, 25, 32767, 2, True, offsets=offsets)
    got = run_case(gpu, (name, layout, "U moves, V stays"), kind, planes, LAYOUTS[layout], want, offsets=offsets, radius=25, threshold=32767, sample=2,
                   blur_first=True, seed=11)
    _, U, V = TS.unpack(got, bits, interleaved, msb)
    assert np.array_equal(V, samples[2]) and not np.array_equal(U, samples[1])


# ---- low bits ----
@pytest.mark.parametrize("layout", ["aligned", "narrow"])
@pytest.mark.parametrize("name", ["p010", "pmsb10"])
def test_the_sources_low_bits_change_no_byte(gpu, name, layout):
    kind = KINDS[name]
    bits, interleaved, msb = kind
    s = TS.shift_of(bits, msb)
    w, h = SIZES[2]
    samples = samples_of(w, h, bits, "soft")
    one, two = packed(samples, kind, 1), packed(samples, kind, 2)
    assert all(np.all(a & ((1 << s) - 1)) and np.all(b & ((1 << s) - 1)) and np.mean(a != b) > 0.5 for a, b in zip(one, two))
    assert all(np.array_equal(a >> s, b >> s) for a, b in zip(one, two))
    want = DS.deband_surfaces(one, bits, interleaved, msb)
    g1 = run_case(gpu, (name, "low bits 1"), kind, one, LAYOUTS[layout], want)
    g2 = run_case(gpu, (name, "low bits 2"), kind, two, LAYOUTS[layout], want)
    for a, b in zip(g1, g2):
        assert np.array_equal(a, b)


# ---- sums that need more than 16 bits ----
@pytest.mark.parametrize("layout", ["aligned", "narrow"])
@pytest.mark.parametrize("pattern", ["all-65535", "checkers", "coin-flips"])
def test_sums_of_four_large_containers(gpu, pattern, layout):
    kind = KINDS["p016"]
    (w, h), n = SIZES[2], 2
    samples, rng = [], np.random.default_rng(65535)
    for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2)):
        y, x = np.arange(ph)[None, :, None], np.arange(pw)[None, None, :]
        f = np.arange(n)[:, None, None]
        p = {"all-65535": lambda: np.full((n, ph, pw), 65535), "checkers": lambda: ((x + y + f) & 1) * 65535,
             "coin-flips": lambda: rng.integers(0, 2, (n, ph, pw)) * 65535}[pattern]()
        samples.append(p.astype(np.uint16))
    planes = TS.pack(tuple(samples), 16, True, True)
    for sample, bf in ((1, True), (2, True), (2, False)):
        for threshold in (32767, 0):
            want = DS.deband_surfaces(planes, 16, True, True, 25, threshold, sample, bf, seed=3)
            if pattern == "coin-flips" and threshold and sample == 2:
                assert set(np.unique(want[1]).tolist()) == {0, 16384, 32768, 49151, 65535}
            run_case(gpu, (pattern, layout, sample, bf, threshold), kind, planes, LAYOUTS[layout], want,
                     radius=25, threshold=threshold, sample=sample, blur_first=bf, seed=3)


# ---- the two routes agree ----
@pytest.mark.parametrize("name", list(KINDS))
def test_the_in_kind_result_is_the_planar_kernels_on_the_same_samples(gpu, name):
    from amatsukaze_amd import Debander
    ctx, torch = gpu
    kind = KINDS[name]
    bits, il, msb = kind
    w, h = SIZES[2]
    planes = packed(samples_of(w, h, bits, "soft"), kind, 9)
    got = run_case(gpu, (name, "in kind"), kind, planes, aligned_layouts, DS.deband_surfaces(planes, bits, il, msb, threshold=2, seed=4), threshold=2, seed=4)
    in_kind = TS.unpack(got, bits, il, msb)
    # the planar LSB copy of the same samples, through amtgpu_deband_run
    pk = (bits, False, False)
    samples = TS.unpack(planes, bits, il, msb)
    n = samples[0].shape[0]
    sl, dl = aligned_layouts(w, h, pk)
    psrc_host = SBuf(n, w, h, pk, **sl).put(samples)
    pdst_host = sentinel_buf(n, w, h, pk, dl)
    psrc, psrc_flat = upload(gpu, psrc_host)
    pdst, pdst_flat = upload(gpu, pdst_host)
    assert psrc.V is not None and not psrc.ref().interleaved and not psrc.ref().msb_aligned
    db = Debander(ctx, (w, h), bits, threshold=2, seed=4)
    assert db.run(psrc, pdst) == n
    db.close()
    torch.cuda.synchronize()
    pgot = download(pdst_host, pdst_flat)
    for k in range(3):
        assert np.array_equal(in_kind[k], pdst_host.view(k, pgot[k])), (name, "plane", k)
    assert any(not np.array_equal(in_kind[k], samples[k]) for k in range(3))
    assert_unchanged(name, psrc_host, psrc_flat)


# ---- planar LSB pairs through the new entry point ----
@pytest.mark.parametrize("layouts", [aligned_layouts, narrow_layouts], ids=["vector", "narrow"])
@pytest.mark.parametrize("bits", [8, 10])
def test_a_planar_lsb_pair_through_the_new_entry_point_is_deband_run(gpu, bits, layouts):
    from amatsukaze_amd import Debander
    ctx, torch = gpu
    kind = PLANAR[bits]
    w, h = SIZES[2]
    samples = samples_of(w, h, bits, "soft")
    n = samples[0].shape[0]
    sl, dl = layouts(w, h, kind)
    src_host = SBuf(n, w, h, kind, **sl).put(samples)
    dst_host = sentinel_buf(n, w, h, kind, dl)
    src, src_flat = upload(gpu, src_host)
    old, old_flat = upload(gpu, dst_host)
    new, new_flat = upload(gpu, dst_host)
    db = Debander(ctx, (w, h), bits)
    s_, old_, new_ = src.ref(), old.ref(), new.ref()
    assert ctx.lib.amtgpu_deband_run(db.h, C.byref(s_), C.byref(old_), n) == 1
    r = ctx.lib.amtgpu_deband_run_surfaces(db.h, C.byref(s_), C.byref(new_), n)
    assert r == 1, ctx.lib.amtgpu_last_error(ctx.h).decode(errors="replace")
    db.close()
    torch.cuda.synchronize()
    one, two = download(dst_host, old_flat), download(dst_host, new_flat)
    for a, b in zip(one, two):
        assert np.array_equal(a, b)
    check_against(("planar", bits), dst_host, two, R.filter_clip(samples, bits))
    assert_unchanged(("planar", bits), src_host, src_flat)


# ---- a clip cut into calls ----
def test_calls_of_2_and_3_frames_give_the_bytes_of_one_call(gpu):
    from amatsukaze_amd import Debander
    ctx, torch = gpu
    kind = KINDS["p010"]
    (w, h), N = SIZES[2], 5
    samples = samples_of(w, h, 10, "soft", N)
    planes = packed(samples, kind, 5)
    want = DS.deband_surfaces(planes, 10, True, True)
    sl, dl = aligned_layouts(w, h, kind)
    src_host = SBuf(N, w, h, kind, **sl).put(planes)
    src, src_flat = upload(gpu, src_host)
    dst_host = sentinel_buf(N, w, h, kind, dl)
    whole, whole_flat = upload(gpu, dst_host)
    parts, parts_flat = upload(gpu, dst_host)
    db = Debander(ctx, (w, h), 10)
    assert db.run(src, whole) == N
    assert db.run(cut(src, 0, 2), cut(parts, 0, 2)) == 2 and db.run(cut(src, 2, 5), cut(parts, 2, 5)) == 3
    db.close()
    torch.cuda.synchronize()
    one, many = download(dst_host, whole_flat), download(dst_host, parts_flat)
    check_against("one call", dst_host, one, want)
    assert any(not np.array_equal(a, b) for a, b in zip(TS.unpack(want, 10, True, True), samples))
    for g1, g2 in zip(one, many):
        assert np.array_equal(g1, g2)
    assert_unchanged("calls", src_host, src_flat)


# ---- the chain on P010: resize, temporal NR, deband ----
def test_the_chain_on_p010_is_the_chain_on_planes(gpu):
    from amatsukaze_amd import Debander, Resizer, temporal_nr
    ctx, torch = gpu
    bits, N, (sw, sh), (w, h) = 10, 8, (48, 36), (32, 24)
    rng = np.random.default_rng(48)
    u = 1 << (bits - 8)
    samples = tuple(((64 + (np.arange(pw)[None, None, :] // 8) * 2) * u + rng.integers(0, 4 * u + 1, (N, ph, pw))).astype(np.uint16)
                    for pw, ph in ((sw, sh), (sw // 2, sh // 2), (sw // 2, sh // 2)))
    results = {}
    for name, kind in (("p010", KINDS["p010"]), ("planar", PLANAR[10])):
        planes = packed(samples, kind, 3) if name == "p010" else samples
        src, _ = upload(gpu, SBuf(N, sw, sh, kind, **aligned_layouts(sw, sh, kind)[0]).put(planes))
        stages = []
        for _ in range(3):
            host = sentinel_buf(N, w, h, kind, aligned_layouts(w, h, kind)[1])
            stages.append((host, *upload(gpu, host)))
        rz, db = Resizer(ctx, (sw, sh), (w, h), bits), Debander(ctx, (w, h), bits, radius=9, threshold=2)
        assert rz.run(src, stages[0][1]) == N
        assert temporal_nr(ctx, stages[0][1], stages[1][1]) == (0, N)
        assert db.run(stages[1][1], stages[2][1]) == N
        rz.close()
        db.close()
        torch.cuda.synchronize()
        host, _, flat = stages[2]
        got = download(host, flat)
        tight = tuple(np.array(host.view(k, got[k])) for k in range(len(got)))
        results[name] = TS.unpack(tight, bits, kind[1], kind[2])
        mid_host, _, mid_flat = stages[1]
        mid = download(mid_host, mid_flat)
        before = TS.unpack(tuple(np.array(mid_host.view(k, mid[k])) for k in range(len(mid))), bits, kind[1], kind[2])
        assert any(not np.array_equal(a, b) for a, b in zip(results[name], before)), (name, "the deband changed nothing")
    for k in range(3):
        assert np.array_equal(results["p010"][k], results["planar"][k]), ("plane", k)


# ---- refusals ----
def test_refusals_write_nothing(gpu):
    from amatsukaze_amd import AmtError, Debander, binding
    ctx, torch = gpu
    N, w, h, radius = 3, 34, 20, 5
    hUV = h // 2
    lib = ctx.lib
    last = lambda: lib.amtgpu_last_error(ctx.h).decode(errors="replace")
    clips = {}

    def pair(name, kind):
        samples = samples_of(w, h, kind[0], "random", N)
        sl, dl = aligned_layouts(w, h, kind)
        sh, dh = SBuf(N, w, h, kind, **sl).put(packed(samples, kind, 1)), sentinel_buf(N, w, h, kind, dl)
        clips[name] = [(sh, *upload(gpu, sh)), (dh, *upload(gpu, dh))]
        return clips[name][0][1].ref(), clips[name][1][1].ref()

    def changed(desc, **kw):
        c = binding.Surfaces()
        C.memmove(C.byref(c), C.byref(desc), C.sizeof(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def call(obj, s_, t_, n):
        r = lib.amtgpu_deband_run_surfaces(obj.h, C.byref(s_), C.byref(t_), n)
        return r, last()

    s, t = pair("nv12", KINDS["nv12"])
    pl8_s, pl8_d = pair("planar8", PLANAR[8])
    p010_s, p010_d = pair("p010", KINDS["p010"])
    il10_s, il10_d = pair("il10", KINDS["il10"])
    pmsb_s, pmsb_d = pair("pmsb10", KINDS["pmsb10"])
    pl10_s, pl10_d = pair("planar10", PLANAR[10])
    assert s.interleaved and s.pitchUV >= w and t.pitchUV >= w
    db = Debander(ctx, (w, h), 8, radius, 32767, 2, True)
    db10 = Debander(ctx, (w, h), 10, radius)
    cases = {
        # name: (arguments..., words the message must hold)
        "NV12 into planes": (db, s, pl8_d, N, "not in kind"),
        "planes into NV12": (db, pl8_s, t, N, "not in kind"),
        "P010 into interleaved LSB": (db10, p010_s, il10_d, N, "not in kind"),
        "interleaved LSB into P010": (db10, il10_s, p010_d, N, "the filter converts no layouts"),
        "P010 into planar MSB": (db10, p010_s, pmsb_d, N, "not in kind"),
        "planar MSB into planar LSB": (db10, pmsb_s, pl10_d, N, "the filter converts no layouts"),
        "planar LSB into planar MSB": (db10, pl10_s, pmsb_d, N, "not in kind"),
        "P010 into NV12": (db10, p010_s, t, N, "destination: 8 bits, the debander was created for 10"),
        "P010 into a descriptor that says P012": (db10, p010_s, changed(p010_d, bits=12), N, "destination: 12 bits, the debander was created for 10"),
        "a P010 pair for the 8-bit object": (db, p010_s, p010_d, N, "source: 10 bits, the debander was created for 8"),
        "an NV12 pair for the 10-bit object": (db10, s, t, N, "source: 8 bits, the debander was created for 10"),
        "interleaved source pitchUV below width": (db, changed(s, pitchUV=w - 2), t, N, "source: pitch smaller than the row"),
        "interleaved destination pitchUV below width": (db, s, changed(t, pitchUV=w - 1), N, "destination: pitch smaller than the row"),
        "source luma pitch below the row": (db10, changed(p010_s, pitchY=w - 2), p010_d, N, "source: pitch smaller than the row"),
        "negative source stride": (db10, changed(p010_s, strideY=-p010_s.strideY), p010_d, N, "source: negative frame stride"),
        "overlapping destination UV frames": (db, s, changed(t, strideUV=(hUV - 1) * t.pitchUV + w - 1), 2, "destination frames overlap each other"),
        "destination is the source": (db, s, s, N, "overlaps the source's"),
        "destination UV inside the source's luma": (db, s, changed(t, U=s.Y), 1, "overlaps the source's"),
        "destination luma on the last byte of the source's UV rows": (db, s, changed(t, Y=s.U + s.strideUV * (N - 1) + (hUV - 1) * s.pitchUV + w - 1), N,
                                                                      "overlaps the source's"),
        "null source UV plane": (db, changed(s, U=None), t, N, "null"),
        "null destination UV plane": (db10, p010_s, changed(p010_d, U=None), N, "null"),
        "MSB-aligned at 8 bits": (db, changed(s, msb_aligned=1), changed(t, msb_aligned=1), N, "MSB"),
        "negative frame count": (db10, p010_s, p010_d, -1, "negative frame count"),
    }
    for what, (*args, words) in cases.items():
        r, msg = call(*args)
        assert r == 0 and "[Deband]" in msg and words in msg, (what, msg)
    assert call(db, s, t, 0)[0] == 1                                    # nothing to filter: 1
    with pytest.raises(AmtError, match="Deband"):
        db.run(clips["nv12"][0][1], clips["planar8"][1][1])             # a mixed pair from Python
    with pytest.raises(AmtError):
        db10.run(clips["p010"][0][1], cut(clips["p010"][1][1], 0, 2))   # more frames than dst holds
    torch.cuda.synchronize()
    for name, both in clips.items():
        for host, _, flat_t in both:
            assert_unchanged(name, host, flat_t)                        # sources as they were, destinations still the sentinel everywhere
    # ... and after all of it the objects filter as they were made to
    for obj, name, (a, b_), params in ((db, "nv12", (s, t), (32767, 2, True)), (db10, "p010", (p010_s, p010_d), (1, 2, True))):
        r, msg = call(obj, a, b_, N)
        assert r == 1, msg
        torch.cuda.synchronize()
        kind = KINDS[name]
        sh, _, sflat = clips[name][0]
        dh, _, dflat = clips[name][1]
        want = DS.deband_surfaces(tuple(sh.view(k) for k in range(2)), kind[0], True, kind[2], radius, *params)
        check_against(("after the refusals", name), dh, download(dh, dflat), want)
        assert_unchanged(name, sh, sflat)
    db.close()
    db10.close()
