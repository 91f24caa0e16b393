"""GPU parity of delogo_kernel on every access path and bit depth.  The kernel has three bodies -- four samples per lane (`quad`), two
(`paired`) and one -- chosen per plane from the width, origin, pitch and base alignment; the logos here select each of them for luma and
for chroma, with rows wide enough for a second and third trip of each body's x loop, workgroups that straddle the Y/U and U/V planes,
frame groups with a ragged tail, odd chroma row counts in field mode under both chroma parities, fades off the 0.1 grid and outside
[0, 1], and 8 / 10 / 12 / 14 / 16 bits with container values above the declared depth.
Every case is compared with the oracle's Delogo frame by frame over whole planes, pitch padding included."""
import numpy as np
import pytest

import amt_synth as S
from amtlib import Oracle, _ptr
from test_gpu_parity import gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

BITS = [8, 10, 12, 14, 16]

# name: W, H, LW, LH, IMGX, IMGY, luma pitch - W, chroma pitch - W/2, plane base offset in samples
#                                                                              luma body          chroma body
LOGOS = {
    "98x50_y18": (352, 240, 98, 50, 224, 18, 32, 16, 0),                     # paired             single (49 wide, 25 rows)
    "98x50_y16": (352, 240, 98, 50, 224, 16, 32, 16, 0),                     #   (the other chroma field parity)
    "100x34_y16": (352, 240, 100, 34, 224, 16, 32, 16, 0),                   # quad               paired (50 wide, 17 rows)
    "100x34_y18": (352, 240, 100, 34, 224, 18, 32, 16, 0),
    "100x34_x226": (352, 240, 100, 34, 226, 16, 32, 16, 0),                  # quad, rows 2 (mod 4)  single (origin 113)
    "520x18": (720, 480, 520, 18, 160, 64, 0, 0, 0),                         # quad, 3 trips      quad (260), 2 trips
    "262x34": (720, 480, 262, 34, 64, 32, 32, 16, 0),                        # paired, 3 trips    single (131), 3 trips
    "96x48_odd_luma_pitch": (352, 240, 96, 48, 224, 18, 33, 16, 0),          # single, 2 trips    quad
    "96x48_odd_pitches": (352, 240, 96, 48, 224, 16, 33, 17, 0),             # single             single
    "96x48_base_plus_1": (352, 240, 96, 48, 224, 18, 32, 16, 1),             # single             single
}


def fades_for(n):
    """27 frames = three full groups of 8 and a tail of 3: group 0 all {0, 0} (the group that leaves the kernel early at 8 and 16 bits);
    group 1 mixes {0, 0} with frame-mode and field-mode pairs of the 0.1 grid; group 2 and the tail are arbitrary floats, some below 0 and
    some above 1.  9 frames = group 1 and one arbitrary pair; 1 frame = a field-mode pair."""
    g0 = [(0.0, 0.0)] * 8
    g1 = [(0.0, 0.0), (1.0, 1.0), (1.0, 0.0), (0.0, 1.0), (0.3, 0.8), (0.0, 0.0), (0.5, 0.5), (0.7, 0.2)]
    rng = np.random.RandomState(27)
    rest = [tuple(rng.uniform(-0.4, 1.6, 2)) for _ in range(11)]
    rest[0] = (-0.3712, -0.3712)
    rest[1] = (1.4349, 0.2183)
    rest[2] = (0.123456, 0.123456)
    rest[3] = (0.91713, -0.2051)
    rest[8] = (1.0000001, 1.0000001)
    rest[9] = (0.0, 3.1e-5)
    rest[10] = (1.5999, 1.5999)
    if n == 27:
        f = g0 + g1 + rest
    elif n == 9:
        f = g1 + rest[1:2]
    else:
        f = [(0.3, 0.8)]
    f = np.array(f, np.float32)
    assert f.shape == (n, 2)
    return f


def make_planes(rng, n, W, H, pY, pUV, bits, rect):
    """noise over the whole depth (so that both ends of Delogo's clamp are met), pitch padding included; inside the rectangle, runs of
    the extreme container values: 0, maxv, the container's top, and above maxv where the container is wider than the depth"""
    maxv = (1 << bits) - 1
    dt = np.uint8 if bits <= 8 else np.uint16
    top = 255 if bits <= 8 else 65535
    x0, y0, lw, lh = rect
    P = {"Y": rng.randint(0, maxv + 1, (n, H, pY)).astype(dt), "U": rng.randint(0, maxv + 1, (n, H // 2, pUV)).astype(dt),
         "V": rng.randint(0, maxv + 1, (n, H // 2, pUV)).astype(dt)}
    specials = [0, maxv, top, min(top, maxv + 1), min(top, 3 * maxv)]
    for name, (px, py, pw, ph) in (("Y", (x0, y0, lw, lh)), ("U", (x0 // 2, y0 // 2, lw // 2, lh // 2)), ("V", (x0 // 2, y0 // 2, lw // 2, lh // 2))):
        for k, v in enumerate(specials):
            r = (2 + 3 * k) % ph
            P[name][:, py + r, px + 1 + k:px + pw - k] = v                   # (odd start, ragged end: every lane position of every body)
        P[name][:, py + ph - 1, px + pw - 1] = top                            # the rectangle's last sample
    return P


def to_dev(gpu, arr, off):
    """arr (n, rows, pitch) on the device with the same strides, its base `off` samples into an allocation"""
    torch = gpu["torch"]
    src = torch.from_numpy(arr if arr.dtype == np.uint8 else arr.view(np.int16))
    flat = torch.zeros(arr.size + off, dtype=src.dtype, device=gpu["dev"])
    t = flat[off:].view(arr.shape)
    t.copy_(src)
    return t


def host(t):
    a = t.cpu().numpy()
    return a if a.dtype == np.uint8 else a.view(np.uint16)


def assert_finite_mix(data, lw, lh, planes, rect, fades, maxv):
    """the reference's float-to-integer conversion of a NaN is undefined, so no case may produce one: fade*bg + (1-fade)*s, restated in
    float32 over every rectangle sample, frame and fade of the case, is finite"""
    x0, y0 = rect[0], rect[1]
    ysz, csz = lw * lh, (lw // 2) * (lh // 2)
    off = [0, 2 * ysz, 2 * ysz + 2 * csz]
    maxv = np.float32(maxv)
    with np.errstate(over="ignore", invalid="ignore"):
        for k, name in enumerate("YUV"):
            pw, ph = (lw, lh) if k == 0 else (lw // 2, lh // 2)
            px, py = (x0, y0) if k == 0 else (x0 // 2, y0 // 2)
            sz = pw * ph
            a = data[off[k]:off[k] + sz].reshape(ph, pw)
            b = data[off[k] + sz:off[k] + 2 * sz].reshape(ph, pw)
            s = planes[name][:, py:py + ph, px:px + pw].astype(np.float32)
            bg = a * s + b * maxv
            for j in range(2):
                f = fades[:, j].astype(np.float32)[:, None, None]
                assert np.isfinite(f * bg + (np.float32(1) - f) * s).all()


def build(gpu, name, bits, n, data=None, seed=0):
    from amatsukaze_amd import AMTEraseLogo, Logo
    W, H, LW, LH, X, Y0, padY, padUV, off = LOGOS[name] if isinstance(name, str) else name
    if data is None:
        data = S.make_logo(LW, LH)[0]
    rng = np.random.RandomState(1000 * bits + n + seed)
    planes = make_planes(rng, n, W, H, W + padY, W // 2 + padUV, bits, (X, Y0, LW, LH))
    fades = fades_for(n)
    assert_finite_mix(data, LW, LH, planes, (X, Y0), fades, (1 << bits) - 1)
    logo = Logo.from_planes(gpu["ctx"], data, LW, LH, W, H, X, Y0)
    orc = Oracle()
    lo = orc.make_logo(data, LW, LH, W, H, X, Y0)
    want = {k: planes[k].copy() for k in "YUV"}
    for i in range(n):
        orc.lib.orc_erase_frame(lo, _ptr(want["Y"][i]), _ptr(want["U"][i]), _ptr(want["V"][i]), W + padY, W // 2 + padUV, bits,
                                float(fades[i, 0]), float(fades[i, 1]))
    # the oracle wrote inside the rectangle only
    for k, (px, py, pw, ph) in (("Y", (X, Y0, LW, LH)), ("U", (X // 2, Y0 // 2, LW // 2, LH // 2)), ("V", (X // 2, Y0 // 2, LW // 2, LH // 2))):
        m = np.ones(planes[k].shape[1:], bool)
        m[py:py + ph, px:px + pw] = False
        assert np.array_equal(want[k][:, m], planes[k][:, m]) and not np.array_equal(want[k], planes[k])
    return dict(W=W, H=H, rect=(X, Y0, LW, LH), off=off, bits=bits, planes=planes, want=want, fades=fades,
                er=AMTEraseLogo(gpu["ctx"], logo), logo=logo)


def device_clip(gpu, cs, planes=None):
    from amatsukaze_amd import DeviceClip
    planes = cs["planes"] if planes is None else planes
    return DeviceClip(*(to_dev(gpu, planes[k], cs["off"]) for k in "YUV"), width=cs["W"], height=cs["H"], bits=cs["bits"])


def assert_planes(clip, want, what):
    for k in "YUV":
        got = host(getattr(clip, k))
        if not np.array_equal(got, want[k]):
            f, y, x = (int(v[0]) for v in np.nonzero(got != want[k]))
            raise AssertionError(f"{what}: plane {k} frame {f} row {y} column {x}: kernel {got[f, y, x]}, oracle {want[k][f, y, x]}, "
                                 f"{int((got != want[k]).sum())} samples differ")


def run_both_entries(gpu, cs):
    """erase_device_fades(src, d_fades, dst): dst == oracle and src untouched; then erase() in place on src == oracle"""
    torch = gpu["torch"]
    src = device_clip(gpu, cs)
    dst = device_clip(gpu, cs)
    d_fades = torch.from_numpy(cs["fades"]).to(gpu["dev"])
    cs["er"].erase_device_fades(src, d_fades, dst=dst)
    gpu["ctx"].synchronize()
    assert_planes(dst, cs["want"], "erase_device_fades(dst)")
    assert_planes(src, cs["planes"], "erase_device_fades(dst) source")
    cs["er"].erase(src, cs["fades"])
    gpu["ctx"].synchronize()
    assert_planes(src, cs["want"], "erase in place")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", sorted(LOGOS))
def test_erase_every_body_27_frames(gpu, name, bits):
    cs = build(gpu, name, bits, 27)
    assert cs["er"].rect[4] == 1
    run_both_entries(gpu, cs)


@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", ["98x50_y18", "100x34_y16", "96x48_base_plus_1", "262x34"])
def test_erase_short_batches(gpu, name, bits, n):
    """one frame, and one full group with a tail of one (the paired body's clamped load of the frames past the end)"""
    run_both_entries(gpu, build(gpu, name, bits, n))


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("corner", ["origin", "bottom_right"])
def test_erase_at_the_frame_corners(gpu, corner, bits):
    """an unpadded frame with the rectangle at (0, 0) and flush with the last sample of every plane"""
    W, H = 352, 240
    x, y = (0, 0) if corner == "origin" else (W - 96, H - 48)
    run_both_entries(gpu, build(gpu, (W, H, 96, 48, x, y, 0, 0, 0), bits, 1))


@pytest.mark.parametrize("odd_pitch", [False, True])
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", ["98x50_y18", "98x50_y16"])
def test_erase_rect_planes(gpu, name, bits, odd_pitch):
    """erase_rect on planes that hold only the rectangle: contiguous (luma paired, chroma single) and with odd row pitches (all single);
    the chroma field parity still comes from the logo's position in the frame"""
    cs = build(gpu, name, bits, 27, seed=5)
    X, Y0, LW, LH = cs["rect"]
    rng = np.random.RandomState(bits)
    maxv = (1 << bits) - 1
    pads = (1, 2) if odd_pitch else (0, 0)                # 98 + 1 and 49 + 2: both odd
    dev, want = {}, {}
    for k, (px, py, pw, ph, pad) in (("Y", (X, Y0, LW, LH, pads[0])), ("U", (X // 2, Y0 // 2, LW // 2, LH // 2, pads[1])),
                                      ("V", (X // 2, Y0 // 2, LW // 2, LH // 2, pads[1]))):
        a = rng.randint(0, maxv + 1, (27, ph, pw + pad)).astype(cs["planes"][k].dtype)
        w = a.copy()
        a[:, :, :pw] = cs["planes"][k][:, py:py + ph, px:px + pw]
        w[:, :, :pw] = cs["want"][k][:, py:py + ph, px:px + pw]
        dev[k], want[k] = to_dev(gpu, a, 0), w
    assert (int(dev["Y"].stride(1)) % 2 == 1) == odd_pitch and (int(dev["U"].stride(1)) % 2 == 1)
    cs["er"].erase_rect(dev["Y"], dev["U"], dev["V"], bits, cs["fades"])
    gpu["ctx"].synchronize()
    for k in "YUV":
        got = host(dev[k])
        assert np.array_equal(got, want[k]), (k, [int(v[0]) for v in np.nonzero(got != want[k])])


@pytest.mark.parametrize("bits", BITS)
def test_erase_logo_whose_fade0_is_not_the_identity(gpu, bits):
    """coefficients that fail the host's |v| < 1e30 test switch the fade-0 skip off (rect[4] == 0): fade-0 frames are then computed like
    any other and must still equal the oracle.  a = 1e30 with b = -1e30 * 200 / maxv keeps a*s + b*maxv finite for every sample."""
    W, H, LW, LH, X, Y0 = LOGOS["98x50_y18"][:6]
    maxv = (1 << bits) - 1
    data = S.make_logo(LW, LH)[0].copy()
    ysz, csz = LW * LH, (LW // 2) * (LH // 2)
    for a_off, sz, pw in ((0, ysz, LW), (2 * ysz, csz, LW // 2), (2 * ysz + 2 * csz, csz, LW // 2)):
        for (r, c) in ((3, 1), (3, 2), (10, pw - 1), (11, 0), (20, 17)):
            data[a_off + r * pw + c] = np.float32(1e30)
            data[a_off + sz + r * pw + c] = np.float32(-1e30) * np.float32(200) / np.float32(maxv)
    cs = build(gpu, "98x50_y18", bits, 27, data=data, seed=9)
    assert cs["er"].rect == (X, Y0, LW, LH, 0)
    assert (cs["fades"][:8] == 0).all()
    run_both_entries(gpu, cs)
