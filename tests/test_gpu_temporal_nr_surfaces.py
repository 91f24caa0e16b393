"""The temporal noise reduction on decoder surfaces on the GPU (amtgpu_temporal_nr_surfaces on NV12 / P010 / P012 / P016 / interleaved
LSB / planar MSB pairs in kind) against its composed numpy restatement (tests/temporal_nr_surfaces_ref.py, which
tests/test_temporal_nr_surfaces_host.py holds against the compiled reference): every container of the destination buffers, the bytes
behind the rows and in front of, between and behind the frames included, on all eight kernel forms; every count of passing frames;
lanes and tails; low bits in and out; planted ties; clip ends, short clips, a clip cut into batches; the planar route on the same
samples; planar LSB pairs through the new entry point; and every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import temporal_nr_ref as R
import temporal_nr_surfaces_ref as TS
from test_gpu_temporal_nr import tie_clip

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
# kind: (bits, interleaved, msb)
KINDS = {"nv12": (8, True, False), "p010": (10, True, True), "p012": (12, True, True), "p016": (16, True, True), "il10": (10, True, False),
         "pmsb10": (10, False, True)}
PLANAR = {8: (8, False, False), 10: (10, False, False)}


class SBuf:
    """a clip of surfaces as flat buffers of containers, one per plane -- (Y, UV) interleaved, (Y, U, V) planar: row y of frame f of plane
    k starts at container off[k] + f * fs[k] + y * pitch[k].  tight_end: the last row of the last frame ends the buffer"""

    def __init__(self, n, w, h, kind, pitch, gap=(0, 0), off=(0, 0, 0), tight_end=False, fill=0):
        self.n, self.w, self.h, self.kind = n, w, h, kind
        self.bits, self.interleaved, self.msb = kind
        self.dt = np.uint8 if self.bits <= 8 else np.uint16
        self.s = TS.shift_of(self.bits, self.msb)
        self.geom, self.flat = [], []
        for k in range(2 if self.interleaved else 3):
            rows, cols, p, g = (h, w, pitch[0], gap[0]) if k == 0 else (h // 2, w if self.interleaved else w // 2, pitch[1], gap[1])
            fs = rows * p + g
            size = off[k] + ((n - 1) * fs + (rows - 1) * p + cols if tight_end else n * fs)
            self.geom.append((rows, cols, p, fs, off[k]))
            self.flat.append(np.full(size, fill, self.dt))

    def view(self, k, flat=None):
        rows, cols, p, fs, off = self.geom[k]
        a = self.flat[k] if flat is None else flat
        es = a.itemsize
        return np.lib.stride_tricks.as_strided(a[off:], (self.n, rows, cols), (fs * es, p * es, es))

    def put(self, planes):
        assert len(planes) == len(self.geom)
        for k, p in enumerate(planes):
            self.view(k)[...] = p
        return self


def aligned_layouts(w, h, kind):
    """(source, destination) layouts on which the kernel takes its 16-byte form: luma rows 16-byte aligned, chroma rows 16-byte aligned
    when interleaved and 8-byte aligned when planar; the two differ in pitches and strides, and the destination has guard containers in
    front of, between and behind its frames"""
    bits, interleaved, _ = kind
    es = 1 if bits <= 8 else 2
    up = lambda v, m: (v + m - 1) // m * m
    ca, cw = (16, w) if interleaved else (8, w // 2)
    pY, pUV = up(w * es, 16) // es, up(cw * es, ca) // es
    src = dict(pitch=(pY, pUV), tight_end=True)
    dst = dict(pitch=(pY + 16 // es, pUV + ca // es), gap=(32 // es, 3 * ca // es), off=(16 // es, ca // es, 2 * ca // es))
    return src, dst


def narrow_layouts(w, h, kind):
    """plane bases one container off and odd pitches: the container-by-container form"""
    cw = w if kind[1] else w // 2
    src = dict(pitch=(w + 1, cw + 1 + cw % 2), gap=(3, 1), off=(1, 1, 1), tight_end=True)
    dst = dict(pitch=(w + 3, cw + 3 + cw % 2), gap=(1, 5), off=(1, 3, 1))
    return src, dst


def half_aligned_layouts(w, h, kind):
    """everything as in aligned_layouts, but the source's chroma rows start 8 bytes off a 16-byte boundary: still the vector form on
    planar MSB surfaces, the narrow one on interleaved surfaces, whose lanes take 16 bytes of a UV row"""
    src, dst = aligned_layouts(w, h, kind)
    es = 1 if kind[0] <= 8 else 2
    up = lambda v, m: (v + m - 1) // m * m
    cw = w if kind[1] else w // 2
    p = up(cw * es, 16) + 8
    src = dict(src, pitch=(src["pitch"][0], p // es))
    return src, dst


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    ctx = Context(0)
    yield ctx, torch
    ctx.close()


def upload(gpu, buf):
    """(DeviceSurfaces over device copies of the buffers -- V None when interleaved --, the flat device tensors)"""
    ctx, torch = gpu
    from amatsukaze_amd import DeviceSurfaces
    dev = torch.device("cuda:0")
    flat_t, views = [], []
    for k, a in enumerate(buf.flat):
        host = np.array(a, copy=True)
        t = torch.from_numpy(host if buf.bits <= 8 else host.view(np.int16)).to(dev)
        rows, cols, p, fs, off = buf.geom[k]
        flat_t.append(t)
        views.append(torch.as_strided(t, (buf.n, rows, cols), (fs, p, 1), off))
    return DeviceSurfaces(views[0], views[1], None if buf.interleaved else views[2], buf.w, buf.h, buf.bits, buf.interleaved, buf.msb), flat_t


def download(buf, flat_t):
    return [t.cpu().numpy().view(buf.dt) for t in flat_t]


def cut(s, i, j):
    from amatsukaze_amd import DeviceSurfaces
    return DeviceSurfaces(s.Y[i:j], s.U[i:j], None if s.V is None else s.V[i:j], s.width, s.height, s.bits, s.interleaved, s.msb)


def sentinel_buf(n, w, h, kind, layout):
    return SBuf(n, w, h, kind, fill=SENTINEL if kind[0] <= 8 else SENTINEL * 0x0101, **{k: v for k, v in layout.items() if k != "tight_end"})


def check_against(what, dst_host, got, want, nout=None):
    """every container of the destination's buffers: the expected frames in the rows' first containers, the sentinel elsewhere"""
    assert len(got) == len(want) == len(dst_host.geom)
    for k in range(len(want)):
        e = np.array(dst_host.flat[k], copy=True)
        dst_host.view(k, e)[:want[k].shape[0] if nout is None else nout] = want[k]
        bad = np.flatnonzero(got[k] != e)
        assert bad.size == 0, (what, "plane", k, bad.size, "containers differ; the first at", int(bad[0]), "got", int(got[k][bad[0]]), "want", int(e[bad[0]]))


def assert_unchanged(what, host, flat_t):
    for g, a in zip(download(host, flat_t), host.flat):
        assert np.array_equal(g, a), (what, "the source changed")


def packed(samples, kind, seed):
    """the surface's tight planes that hold these samples, random non-zero low bits in every container where the kind has any"""
    bits, interleaved, msb = kind
    planes = TS.pack(samples, bits, interleaved, msb, np.random.default_rng(seed))
    s = TS.shift_of(bits, msb)
    if s:
        assert all(np.all(p & ((1 << s) - 1)) for p in planes)                   # on the input: every container has low bits
    return planes


def run_whole_clip(gpu, what, kind, planes, d, thr, il, layouts, want=None):
    """filters the whole clip in one call and compares every destination container; the sources must stay as they were.  Returns the
    destination's buffers"""
    from amatsukaze_amd import temporal_nr
    ctx, torch = gpu
    bits, interleaved, msb = kind
    n, h, w = planes[0].shape
    if want is None:
        want, _ = TS.filter_surfaces(planes, d, thr, bits, interleaved, msb, il)
    sl, dl = layouts(w, h, kind)
    src_host = SBuf(n, w, h, kind, **sl).put(planes)
    dst_host = sentinel_buf(n, w, h, kind, dl)
    src, src_flat = upload(gpu, src_host)
    dst, dst_flat = upload(gpu, dst_host)
    assert (src.V is None) == interleaved
    assert temporal_nr(ctx, src, dst, distance=d, threshold=thr, interlaced=il) == (0, n)
    torch.cuda.synchronize()
    got = download(dst_host, dst_flat)
    check_against(what, dst_host, got, want)
    assert_unchanged(what, src_host, src_flat)
    low = (1 << TS.shift_of(bits, msb)) - 1
    for k in range(len(want)):
        assert not np.any(dst_host.view(k, got[k]) & low), (what, "low bits in the output")
    return got


# ---- every count of passing frames ----
@functools.lru_cache(maxsize=None)
def count_case(name):
    """make_clip(12, 34, 8, ...) at the kind's depth, packed: (planes, want, count, the samples); computed once and read-only"""
    kind = KINDS[name]
    bits, interleaved, msb = kind
    samples = R.make_clip(12, 34, 8, bits, 1, np.random.default_rng(bits * 13 + 5))
    planes = packed(samples, kind, bits)
    want, count = TS.filter_surfaces(planes, 3, 1, bits, interleaved, msb)
    for a in (*planes, *want, count):
        a.setflags(write=False)
    return planes, want, count, samples


@pytest.mark.parametrize("name", list(KINDS))
def test_every_count_of_passing_frames(gpu, name):
    kind = KINDS[name]
    bits, interleaved, msb = kind
    planes, want, count, samples = count_case(name)
    # the generator's conditions, before the GPU result is looked at
    assert set(np.unique(count)) == set(range(1, 8)), sorted(np.unique(count))
    for k, (a, b) in enumerate(zip(TS.unpack(want, bits, interleaved, msb), samples)):
        changed = float(np.mean(a != b))
        print(name, "plane", k, "changed %.1f %%" % (100 * changed))
        assert changed >= 0.05, (k, changed)
    run_whole_clip(gpu, name, kind, planes, 3, 1, False, aligned_layouts, want)


# ---- shapes: 16-byte lanes with every tail, the narrow form, both chroma mappings ----
@functools.lru_cache(maxsize=None)
def shape_clip(w, h, name, seed=0):
    kind = KINDS[name]
    bits, interleaved, msb = kind
    samples = R.make_clip(8, w, h, bits, 1, np.random.default_rng(w * 131 + h * 7 + bits + seed))
    if name == "il10":
        samples[0][3, h - 1, w - 1] = 0xFC00                   # containers above maxv in an LSB surface: taken as stored
        samples[1][4, 0, 0] = 0xFFFF
        samples[2][2, h // 2 - 1, w // 2 - 1] = 0x0400
    planes = packed(samples, kind, w + h + seed)
    for p in planes:
        p.setflags(write=False)
    return planes


@pytest.mark.parametrize("interlaced", [False, True], ids=["progressive", "interlaced"])
@pytest.mark.parametrize("h", [4, 8, 12])
@pytest.mark.parametrize("w", [2, 6, 34, 66, 130])
@pytest.mark.parametrize("name", list(KINDS))
def test_vector_lanes_with_every_tail(gpu, name, w, h, interlaced):
    run_whole_clip(gpu, (name, w, h, interlaced), KINDS[name], shape_clip(w, h, name), 3, 1, interlaced, aligned_layouts)


@pytest.mark.parametrize("interlaced", [False, True], ids=["progressive", "interlaced"])
@pytest.mark.parametrize("h", [4, 12])
@pytest.mark.parametrize("name", list(KINDS))
def test_the_narrow_form_on_unaligned_planes(gpu, name, h, interlaced):
    run_whole_clip(gpu, (name, 18, h, interlaced), KINDS[name], shape_clip(18, h, name), 3, 1, interlaced, narrow_layouts)


@pytest.mark.parametrize("name", ["nv12", "p010", "pmsb10"])
def test_chroma_rows_eight_bytes_off_a_16_byte_boundary(gpu, name):
    run_whole_clip(gpu, (name, "UV rows 8 bytes off"), KINDS[name], shape_clip(34, 8, name), 3, 1, False, half_aligned_layouts)


# ---- low bits ----
@pytest.mark.parametrize("layouts", [aligned_layouts, narrow_layouts], ids=["vector", "narrow"])
@pytest.mark.parametrize("name", ["p010", "p012", "pmsb10"])
def test_the_sources_low_bits_change_no_byte(gpu, name, layouts):
    kind = KINDS[name]
    bits, interleaved, msb = kind
    s = TS.shift_of(bits, msb)
    samples = R.make_clip(8, 34, 8, bits, 1, np.random.default_rng(bits))
    one, two = packed(samples, kind, 1), packed(samples, kind, 2)
    assert all(np.all(a & ((1 << s) - 1)) and np.all(b & ((1 << s) - 1)) and np.mean(a != b) > 0.5 for a, b in zip(one, two))
    assert all(np.array_equal(a >> s, b >> s) for a, b in zip(one, two))
    g1 = run_whole_clip(gpu, (name, "low bits 1"), kind, one, 3, 1, False, layouts)
    g2 = run_whole_clip(gpu, (name, "low bits 2"), kind, two, 3, 1, False, layouts)
    for a, b in zip(g1, g2):
        assert np.array_equal(a, b)


# ---- planted ties: the pixels whose byte depends on how the sum is formed ----
@pytest.mark.parametrize("name, bits, d", [("nv12", 8, 3), ("p010", 10, 3), ("p016", 16, 3)])
def test_planted_ties(gpu, name, bits, d):
    kind = KINDS[name]
    assert kind[0] == bits
    thr = 3 * d                                                  # tie_search's clips need it
    samples, want, differ = tie_clip(bits, d, thr)
    assert np.all(want[3][d] == 2 * d)                           # count 6 at every pixel of the centre frame
    for k in range(3):                                           # whose samples sum to 3 mod 6 in every plane
        P = samples[k].astype(np.int64)
        assert np.all(np.sum(P * (np.abs(P - P[d]) <= d << (bits - 8)), axis=0) % (2 * d) == d)
    print(name, "count", 2 * d, "pixels of the centre frame where a wrong variant's byte differs:", differ)
    assert differ["fma"] >= 8, differ
    if bits == 8 and d == 3:
        assert differ["rational"] >= 8 and differ["reversed"] >= 8, differ
    else:
        for v in ("rational", "reversed"):
            if differ[v] < 8:
                print("  condition dropped at %d bits, count %d: the search found %d pixels for the %s variant" % (bits, 2 * d, differ[v], v))
    planes = packed(samples, kind, bits + d)
    packed_want = TS.pack(want[:3], bits, kind[1], kind[2])
    assert all(np.array_equal(a, b) for a, b in zip(packed_want, TS.filter_surfaces(planes, d, thr, bits, kind[1], kind[2])[0]))
    run_whole_clip(gpu, ("ties", name, d), kind, planes, d, thr, False, aligned_layouts, packed_want)


# ---- parameters ----
@pytest.mark.parametrize("thr", [0, 1, 3, 255])
@pytest.mark.parametrize("d", [0, 1, 3, 5])
def test_distances_and_thresholds(gpu, d, thr):
    samples = R.make_clip(13, 34, 8, 8, max(1, min(thr, 3)), np.random.default_rng(d * 17 + thr))
    run_whole_clip(gpu, (d, thr), KINDS["nv12"], packed(samples, KINDS["nv12"], 0), d, thr, False, aligned_layouts)


def test_the_largest_distance(gpu):
    samples = R.make_clip(130, 4, 4, 8, 1, np.random.default_rng(63))
    planes = packed(samples, KINDS["nv12"], 0)
    want, count = TS.filter_surfaces(planes, 63, 1, 8, True, False)
    assert int(count.max()) >= 64                                # counts the short windows never reach
    run_whole_clip(gpu, "d = 63", KINDS["nv12"], planes, 63, 1, False, aligned_layouts, want)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7])
@pytest.mark.parametrize("name", ["nv12", "p010"])
def test_short_clips_follow_the_clamp_rule(gpu, name, n):
    kind = KINDS[name]
    samples = R.make_clip(n, 34, 8, kind[0], 1, np.random.default_rng(n))
    run_whole_clip(gpu, ("clip_frames", name, n), kind, packed(samples, kind, n), 3, 1, False, aligned_layouts)


# ---- a clip cut into batches ----
def test_batches_with_halos_give_the_bytes_of_one_call(gpu):
    from amatsukaze_amd import temporal_nr
    ctx, torch = gpu
    kind = KINDS["p010"]
    N, w, h, d, thr = 20, 34, 8, 3, 1
    planes = packed(R.make_clip(N, w, h, 10, thr, np.random.default_rng(20)), kind, 20)
    want, _ = TS.filter_surfaces(planes, d, thr, 10, True, True)
    sl, dl = aligned_layouts(w, h, kind)
    src_host = SBuf(N, w, h, kind, **sl).put(planes)
    src, src_flat = upload(gpu, src_host)
    dst_host = sentinel_buf(N, w, h, kind, dl)
    whole, whole_flat = upload(gpu, dst_host)
    parts, parts_flat = upload(gpu, dst_host)
    assert temporal_nr(ctx, src, whole, d, thr) == (0, N)
    for lo in range(0, N, 6):
        hi = min(N, lo + 6)
        a, b = max(0, lo - d), min(N, hi + d)
        # (a middle batch: the defaults are its own frames; the last batch's halo is the clip's end, whose frames the defaults would add)
        frames = {} if 0 < a and b < N else dict(out_first=lo, nout=hi - lo)
        assert temporal_nr(ctx, cut(src, a, b), cut(parts, lo, hi), d, thr, src_first=a, clip_frames=N, **frames) == (lo, hi - lo)
    torch.cuda.synchronize()
    one, many = download(dst_host, whole_flat), download(dst_host, parts_flat)
    check_against("one call", dst_host, one, want)
    check_against("four calls", dst_host, many, want)
    assert_unchanged("batches", src_host, src_flat)


# ---- the two routes agree ----
@pytest.mark.parametrize("interlaced", [False, True], ids=["progressive", "interlaced"])
@pytest.mark.parametrize("name", list(KINDS))
def test_the_in_kind_result_is_the_planar_kernels_on_the_same_samples(gpu, name, interlaced):
    from amatsukaze_amd import temporal_nr
    ctx, torch = gpu
    kind = KINDS[name]
    bits, il, msb = kind
    planes = shape_clip(66, 8, name, seed=1)
    got = run_whole_clip(gpu, (name, "in kind"), kind, planes, 3, 1, interlaced, aligned_layouts)
    n, h, w = planes[0].shape
    dst_host = sentinel_buf(n, w, h, kind, aligned_layouts(w, h, kind)[1])
    in_kind = TS.unpack(tuple(dst_host.view(k, got[k]) for k in range(len(got))), bits, il, msb)
    # the planar LSB copy of the same samples, through amtgpu_temporal_nr
    pk = (bits, False, False)
    samples = TS.unpack(planes, bits, il, msb)
    sl, dl = aligned_layouts(w, h, pk)
    psrc_host = SBuf(n, w, h, pk, **sl).put(samples)
    pdst_host = sentinel_buf(n, w, h, pk, dl)
    psrc, psrc_flat = upload(gpu, psrc_host)
    pdst, pdst_flat = upload(gpu, pdst_host)
    assert psrc.V is not None and not psrc.ref().interleaved and not psrc.ref().msb_aligned
    assert temporal_nr(ctx, psrc, pdst, 3, 1, interlaced) == (0, n)
    torch.cuda.synchronize()
    pgot = download(pdst_host, pdst_flat)
    for k in range(3):
        assert np.array_equal(in_kind[k], pdst_host.view(k, pgot[k])), (name, "plane", k)
    assert_unchanged(name, psrc_host, psrc_flat)


# ---- planar LSB pairs through the new entry point ----
def raw(ctx, fn, s_, src_first, nsrc, clip, w_, h_, out_first, nout, d, thr, il, t_):
    r = fn(ctx.h, C.byref(s_), src_first, nsrc, clip, w_, h_, out_first, nout, d, thr, il, C.byref(t_))
    return r, ctx.lib.amtgpu_last_error(ctx.h).decode(errors="replace")


@pytest.mark.parametrize("layouts", [aligned_layouts, narrow_layouts], ids=["vector", "narrow"])
@pytest.mark.parametrize("bits", [8, 10])
def test_a_planar_lsb_pair_through_the_new_entry_point_is_temporal_nr(gpu, bits, layouts):
    ctx, torch = gpu
    kind = PLANAR[bits]
    n, w, h = 8, 34, 8
    samples = R.make_clip(n, w, h, bits, 1, np.random.default_rng(bits + 40))
    sl, dl = layouts(w, h, kind)
    src_host = SBuf(n, w, h, kind, **sl).put(samples)
    dst_host = sentinel_buf(n, w, h, kind, dl)
    src, src_flat = upload(gpu, src_host)
    old, old_flat = upload(gpu, dst_host)
    new, new_flat = upload(gpu, dst_host)
    assert raw(ctx, ctx.lib.amtgpu_temporal_nr, src.ref(), 0, n, n, w, h, 0, n, 3, 1, 0, old.ref())[0] == 1
    r, msg = raw(ctx, ctx.lib.amtgpu_temporal_nr_surfaces, src.ref(), 0, n, n, w, h, 0, n, 3, 1, 0, new.ref())
    assert r == 1, msg
    torch.cuda.synchronize()
    one, two = download(dst_host, old_flat), download(dst_host, new_flat)
    for a, b in zip(one, two):
        assert np.array_equal(a, b)
    check_against(("planar", bits), dst_host, two, R.filter_clip(samples, 3, 1, bits)[:3])
    assert_unchanged(("planar", bits), src_host, src_flat)


# ---- refusals ----
def test_refusals_launch_nothing(gpu):
    from amatsukaze_amd import AmtError, binding, temporal_nr
    ctx, torch = gpu
    N, w, h = 8, 34, 8
    hUV = h // 2
    clips = {}

    def pair(name, kind):
        samples = R.make_clip(N, w, h, kind[0], 1, np.random.default_rng(len(name)))
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

    s, t = pair("nv12", KINDS["nv12"])
    pl8_s, pl8_d = pair("planar8", PLANAR[8])
    p010_s, p010_d = pair("p010", KINDS["p010"])
    il10_s, il10_d = pair("il10", KINDS["il10"])
    pmsb_s, pmsb_d = pair("pmsb10", KINDS["pmsb10"])
    pl10_s, pl10_d = pair("planar10", PLANAR[10])
    mid = cut(clips["nv12"][0][1], 2, 6).ref()                   # frames 2..5 of the clip of 8
    assert s.interleaved and s.pitchUV >= w and t.pitchUV >= w
    last_uv_byte = s.U + s.strideUV * (N - 1) + (hUV - 1) * s.pitchUV + w - 1        # of the source's UV rows of `width` containers
    cases = {
        # name: (arguments, a word the message must hold)
        "NV12 into planes": ((s, 0, N, N, w, h, 0, N, 3, 1, 0, pl8_d), "not in kind"),
        "planes into NV12": ((pl8_s, 0, N, N, w, h, 0, N, 3, 1, 0, t), "not in kind"),
        "P010 into interleaved LSB": ((p010_s, 0, N, N, w, h, 0, N, 3, 1, 0, il10_d), "not in kind"),
        "interleaved LSB into P010": ((il10_s, 0, N, N, w, h, 0, N, 3, 1, 0, p010_d), "not in kind"),
        "P010 into planar MSB": ((p010_s, 0, N, N, w, h, 0, N, 3, 1, 0, pmsb_d), "not in kind"),
        "planar MSB into planar LSB": ((pmsb_s, 0, N, N, w, h, 0, N, 3, 1, 0, pl10_d), "converts no layouts"),
        "planar LSB into planar MSB": ((pl10_s, 0, N, N, w, h, 0, N, 3, 1, 0, pmsb_d), "converts no layouts"),
        "P010 into NV12": ((p010_s, 0, N, N, w, h, 0, N, 3, 1, 0, t), "bits"),
        "P010 into a descriptor that says P012": ((p010_s, 0, N, N, w, h, 0, N, 3, 1, 0, changed(p010_d, bits=12)), "bits"),
        "interleaved source pitchUV below width": ((changed(s, pitchUV=w - 2), 0, N, N, w, h, 0, N, 3, 1, 0, t), "source: pitch smaller than the row"),
        "interleaved destination pitchUV below width": ((s, 0, N, N, w, h, 0, N, 3, 1, 0, changed(t, pitchUV=w - 1)), "destination: pitch smaller than the row"),
        "destination is the source": ((s, 0, N, N, w, h, 0, N, 3, 1, 0, s), "overlaps the source's"),
        "destination UV inside the source's luma": ((s, 0, N, N, w, h, 0, 1, 3, 1, 0, changed(t, U=s.Y)), "overlaps the source's"),
        "destination luma on the last byte of the source's UV rows": ((s, 0, N, N, w, h, 0, 1, 3, 1, 0, changed(t, Y=last_uv_byte)), "overlaps the source's"),
        "overlapping destination UV frames": ((s, 0, N, N, w, h, 0, 2, 3, 1, 0, changed(t, strideUV=(hUV - 1) * t.pitchUV + w - 1)), "destination frames overlap each other"),
        "negative source stride": ((changed(p010_s, strideY=-p010_s.strideY), 0, N, N, w, h, 0, N, 3, 1, 0, p010_d), "source: negative frame stride"),
        "negative destination UV stride": ((s, 0, N, N, w, h, 0, N, 3, 1, 0, changed(t, strideUV=-t.strideUV)), "destination: negative frame stride"),
        "temporal_distance 64": ((s, 0, N, N, w, h, 0, N, 64, 1, 0, t), "temporal_distance"),
        "threshold -1": ((p010_s, 0, N, N, w, h, 0, N, 3, -1, 0, p010_d), "threshold"),
        "bits 7": ((changed(s, bits=7), 0, N, N, w, h, 0, N, 3, 1, 0, changed(t, bits=7)), "bits"),
        "MSB-aligned at 8 bits": ((changed(s, msb_aligned=1), 0, N, N, w, h, 0, N, 3, 1, 0, changed(t, msb_aligned=1)), "MSB"),
        "odd width": ((s, 0, N, N, w - 1, h, 0, N, 3, 1, 0, t), "even"),
        "interlaced with height % 4 == 2": ((p010_s, 0, N, N, w, h - 2, 0, N, 3, 1, 1, p010_d), "multiple of 4"),
        "source luma pitch below the row": ((changed(s, pitchY=w - 2), 0, N, N, w, h, 0, N, 3, 1, 0, t), "source: pitch smaller than the row"),
        "null UV plane": ((changed(s, U=None), 0, N, N, w, h, 0, N, 3, 1, 0, t), "null"),
        "window frame before the batch": ((mid, 2, 4, N, w, h, 4, 1, 3, 1, 0, t), "window frame 1 "),
        "window frame behind the batch": ((mid, 2, 4, N, w, h, 5, 1, 1, 1, 0, t), "window frame 6 "),
        "output frame behind the clip": ((s, 0, N, N, w, h, N - 1, 2, 0, 1, 0, t), "outside the clip"),
        "negative output count": ((pmsb_s, 0, N, N, w, h, 0, -1, 3, 1, 0, pmsb_d), "negative"),
    }
    fn = ctx.lib.amtgpu_temporal_nr_surfaces
    for what, (args, word) in cases.items():
        r, msg = raw(ctx, fn, *args)
        assert r == 0 and msg.strip() and "[TemporalNR]" in msg and word in msg, (what, msg)
    assert raw(ctx, fn, s, 0, N, N, w, h, 0, 0, 3, 1, 0, t)[0] == 1                                  # nothing to filter: 1
    with pytest.raises(AmtError, match="TemporalNR"):
        temporal_nr(ctx, clips["nv12"][0][1], clips["planar8"][1][1])                                # a mixed pair from Python
    with pytest.raises(AmtError):
        temporal_nr(ctx, clips["p010"][0][1], cut(clips["p010"][1][1], 0, 3))                        # more output frames than dst holds
    torch.cuda.synchronize()
    for name, both in clips.items():
        for host, _, flat_t in both:
            assert_unchanged(name, host, flat_t)                 # sources as they were, destinations still the sentinel everywhere
    # what the window refusals above lacked is all there at d = 1: frames 3 and 4 from the batch 2..5
    r, msg = raw(ctx, fn, mid, 2, 4, N, w, h, 3, 2, 1, 1, 0, t)
    assert r == 1, msg
    torch.cuda.synchronize()
    sh, _, _ = clips["nv12"][0]
    dh, _, dflat = clips["nv12"][1]
    want, _ = TS.filter_surfaces(tuple(sh.view(k) for k in range(2)), 1, 1, 8, True, False, frames=[3, 4])
    check_against("frames 3 and 4", dh, download(dh, dflat), want)
