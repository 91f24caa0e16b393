"""Automatic logo detection on the HIP path (logofind_kernels.hip, amt_gpu_logofind.hip): the device sums are the numpy statement's
(tests/logofind_ref.py) to the last bit, the synthetic clip's logo is found, and ScanLogo fed with it gives the same .lgd as ScanLogo
given the found rectangle by hand -- on one device, from a raw clip file and over two sharded ranks."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

import amt_synth as S
import logofind_ref as LF
from amtlib import write_raw_clip

pytestmark = pytest.mark.gpu

# the detection clip: a 128 x 64 logo in a 640 x 360 frame, present in half of the frames, flat-background frames for ScanLogo
W, H, LW, LH, X, Y0, N = 640, 360, 128, 64, 480, 32, 240
SEED, PERIOD, FADE, FLAT = 0x5EED00A1, 60, 6, 4


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return dict(torch=torch, ctx=Context(0), dev=torch.device("cuda:0"))


_clips = {}


def synth(bits=8, logo=True):
    key = (bits, logo)
    if key not in _clips:
        data, alpha, aUV = S.make_logo(LW, LH)
        a = alpha if logo else np.zeros_like(alpha)
        au = aUV if logo else np.zeros_like(aUV)
        _clips[key] = S.make_clip_np(N, W, H, SEED, a, au, X, Y0, bits=bits, period=PERIOD, fade=FADE, flat_every=FLAT)
    return _clips[key]


def to_dev(gpu, a):
    t = gpu["torch"].from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
    return t.to(gpu["dev"])


def dclip_of(gpu, clip, bits=8):
    from amatsukaze_amd import DeviceClip
    return DeviceClip(*(to_dev(gpu, clip[k]) for k in "YUV"), width=W, height=H, bits=bits)


def device_sums(gpu, Y, w, h, bits, chunks=None):
    from amatsukaze_amd import LogoFinder
    lf = LogoFinder(gpu["ctx"], w, h, bits)
    dY = to_dev(gpu, Y)
    n = Y.shape[0]
    for a, b in (chunks or [(0, n)]):
        lf.add_device(dY[a:b])
    S1, SM = lf.sums()
    assert lf.nframes == n
    return np.concatenate([S1.ravel(), SM.ravel()])


@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("w,h,pitch,n", [(3, 3, 3, 5), (61, 37, 61, 23), (61, 37, 72, 23), (600, 20, 640, 17), (517, 13, 517, 9),
                                         (250, 9, 256, 33)])
def test_sums_match_numpy(gpu, bits, w, h, pitch, n):
    """unpadded and padded pitch, odd widths, a 3 x 3 frame, rows wider than one wave's span (248 columns): the DPP neighbours across
    waves; whole clip in one call, in ragged chunks and frame by frame -- all byte-equal to the numpy sums"""
    maxv = (1 << bits) - 1
    rng = np.random.RandomState(bits * 1000 + w + pitch)
    Y = rng.randint(0, maxv + 1, size=(n, h, pitch)).astype(np.uint8 if bits == 8 else np.uint16)
    want = LF.sums(Y, w, h)
    assert device_sums(gpu, Y, w, h, bits).tobytes() == want.tobytes()
    chunks = [(a, min(n, a + 7)) for a in range(0, n, 7)]            # the last chunk is ragged
    assert device_sums(gpu, Y, w, h, bits, chunks).tobytes() == want.tobytes()
    assert device_sums(gpu, Y, w, h, bits, [(i, i + 1) for i in range(n)]).tobytes() == want.tobytes()


def test_launch_split_at_16_bits(gpu):
    """16 bits, every horizontal and vertical term at maxv: a batch longer than one launch's 16 384 frames is split so that the
    32-bit partials never wrap"""
    w, h, n, maxv = 64, 8, 16384 * 2 + 5, 65535
    yy, xx = np.mgrid[0:h, 0:w]
    frame = np.where(((xx // 2) + (yy // 2)) % 2 == 0, maxv, 0).astype(np.uint16)
    Y = np.broadcast_to(frame, (n, h, w))
    one = LF.sums(Y[:1], w, h)
    assert one.reshape(2, h, w)[1, 1:-1, 1:-1].min() == 2 * maxv                  # the largest per-frame SM there is
    want = one * n
    got = device_sums(gpu, np.ascontiguousarray(Y), w, h, 16)
    assert got.tobytes() == want.tobytes()


def _alpha_box():
    _, alpha, _ = S.make_logo(LW, LH)
    ys, xs = np.nonzero(alpha > 0)
    return X + xs.min(), Y0 + ys.min(), X + xs.max(), Y0 + ys.max()


def test_detects_the_synthetic_logo(gpu):
    from amatsukaze_amd import LogoFinder
    vis = S.logo_presence(np.arange(N), PERIOD, FADE)
    assert (vis == 0).mean() >= 0.4
    ax0, ay0, ax1, ay1 = _alpha_box()
    rects = {}
    for bits in (8, 10):
        clip = synth(bits)
        lf = LogoFinder(gpu["ctx"], W, H, bits)
        lf.add(dclip_of(gpu, clip, bits))
        S1, SM = lf.sums()
        assert np.concatenate([S1.ravel(), SM.ravel()]).tobytes() == LF.sums(clip["Y"], W, H).tobytes()
        cands = lf.candidates()
        assert cands, "no candidate"
        c = cands[0]
        assert c.imgx <= ax0 and c.imgy <= ay0 and c.imgx + c.w > ax1 and c.imgy + c.h > ay1, (c, (ax0, ay0, ax1, ay1))
        assert c.imgx >= X and c.imgy >= Y0 and c.imgx + c.w <= X + LW and c.imgy + c.h <= Y0 + LH, c
        assert all(c.score >= o.score for o in cands)
        rects[bits] = (c.imgx, c.imgy, c.w, c.h)
        # set_sums round trip: the same candidates from sums put back
        lf2 = LogoFinder(gpu["ctx"], W, H, bits)
        lf2.set_sums(S1, SM, lf.nframes)
        assert lf2.candidates() == cands
    assert rects[8] == rects[10]


def test_logo_free_clip_finds_nothing(gpu, tmp_path):
    from amatsukaze_amd import LogoFinder, ScanLogoAuto
    clip = synth(8, logo=False)
    dclip = dclip_of(gpu, clip)
    lf = LogoFinder(gpu["ctx"], W, H, 8)
    lf.add(dclip)
    assert lf.candidates() == []
    dst = tmp_path / "none.lgd"
    ok, found = ScanLogoAuto(gpu["ctx"], dclip, 1041, dst, 12, 25)
    assert not ok and found is None
    assert gpu["ctx"].lib.amtgpu_last_error(gpu["ctx"].h) == b"no logo found"
    assert not dst.exists()
    # the raw struct is zeroed too
    from amatsukaze_amd import binding
    r = binding.LogoRect(1, 2, 3, 4, 5.0, 6.0, 7, 8)
    cb = binding.CB(lambda *a: 1)
    assert gpu["ctx"].lib.amtgpu_scanlogo_auto(gpu["ctx"].h, C.c_void_p(dclip.Y.data_ptr()), C.c_void_p(dclip.U.data_ptr()),
                                               C.c_void_p(dclip.V.data_ptr()), dclip.strideY, dclip.strideUV, dclip.pitchY, dclip.pitchUV,
                                               W, H, N, 1, str(dst).encode(), 12, 25, cb, None, C.byref(r)) == 0
    assert (r.imgx, r.imgy, r.w, r.h, r.score, r.coherence, r.edge_pixels, r.reserved) == (0, 0, 0, 0, 0.0, 0.0, 0, 0)


def test_refused_device_arguments(gpu):
    lib, ctx = gpu["ctx"].lib, gpu["ctx"]
    for args in ((2, 10, 8), (10, 2, 8), (10, 10, 7), (10, 10, 17)):
        assert not lib.amtgpu_logofind_create(ctx.h, *args)
    h = lib.amtgpu_logofind_create(ctx.h, 16, 8, 8)
    assert h
    try:
        assert lib.amtgpu_logofind_add_batch(h, None, 128, 16, 1) == 0
        assert lib.amtgpu_logofind_add_batch(h, None, 128, 16, -1) == 0
        assert lib.amtgpu_logofind_add_batch(h, None, 128, 16, 0) == 1 and lib.amtgpu_logofind_nframes(h) == 0
        assert lib.amtgpu_logofind_set_sums(h, None, 0) == 0
        s = np.zeros(2 * 16 * 8, np.int64)
        assert lib.amtgpu_logofind_set_sums(h, s.ctypes.data_as(C.c_void_p), -1) == 0
        assert lib.amtgpu_logofind_get_sums(h, None) == 0
        n = C.c_int()
        assert lib.amtgpu_logofind_candidates(h, None, None, -1, C.byref(n)) == 0
        assert lib.amtgpu_logofind_candidates(h, None, None, 0, C.byref(n)) == 1 and n.value == 0
        assert lib.amtgpu_logofind_allreduce(h, None) == 0
    finally:
        lib.amtgpu_logofind_destroy(h)


def test_scanlogo_auto_equals_scanlogo_on_the_found_rectangle(gpu, tmp_path):
    from amatsukaze_amd import ScanLogo, ScanLogoAuto, ScanLogoFileAuto
    clip = synth(8)
    dclip = dclip_of(gpu, clip)
    auto = tmp_path / "auto.lgd"
    ok, r = ScanLogoAuto(gpu["ctx"], dclip, 1041, auto, 12, 25)
    assert ok, gpu["ctx"].lib.amtgpu_last_error(gpu["ctx"].h)
    manual = tmp_path / "manual.lgd"
    assert ScanLogo(gpu["ctx"], dclip, 1041, manual, r.imgx, r.imgy, r.w, r.h, 12, 25)
    assert auto.read_bytes() == manual.read_bytes()
    from amatsukaze_amd import Logo
    info = Logo.load(gpu["ctx"], auto).info                      # the .lgd header carries the found rectangle
    assert (info["imgx"], info["imgy"], info["w"], info["h"], info["imgw"], info["imgh"]) == (r.imgx, r.imgy, r.w, r.h, W, H)
    raw = tmp_path / "clip.amtr"
    write_raw_clip(raw, clip["Y"], clip["U"], clip["V"], W, H)
    fauto = tmp_path / "file_auto.lgd"
    ok, rf = ScanLogoFileAuto(gpu["ctx"], raw, 1041, tmp_path / "work", fauto, 12, 25)
    assert ok, gpu["ctx"].lib.amtgpu_last_error(gpu["ctx"].h)
    assert rf == r and fauto.read_bytes() == auto.read_bytes()


def test_erase_quality_with_the_auto_logo(gpu, tmp_path):
    """logo-present frames erased (fade 1) with the automatically found logo are as close to the logo-free background as with the
    logo ScanLogo makes from the generator's own rectangle: mean absolute error within 1.1 x"""
    from amatsukaze_amd import AMTEraseLogo, Logo, ScanLogo, ScanLogoAuto
    clip = synth(8)
    bg = synth(8, logo=False)["Y"]
    vis = S.logo_presence(np.arange(N), PERIOD, FADE)
    on = np.nonzero(vis >= 1.0)[0]
    assert len(on) > 50
    auto, manual = tmp_path / "auto.lgd", tmp_path / "manual.lgd"
    ok, r = ScanLogoAuto(gpu["ctx"], dclip_of(gpu, clip), 1041, auto, 12, 25)
    assert ok
    assert ScanLogo(gpu["ctx"], dclip_of(gpu, clip), 1041, manual, X, Y0, LW, LH, 12, 25)
    err = {}
    for tag, path in (("auto", auto), ("manual", manual)):
        sub = {k: np.ascontiguousarray(clip[k][on]) for k in "YUV"}
        d = dclip_of(gpu, sub)
        AMTEraseLogo(gpu["ctx"], Logo.load(gpu["ctx"], path)).erase(d, np.ones((len(on), 2), np.float32))
        got = d.Y.cpu().numpy()[:, Y0:Y0 + LH, X:X + LW].astype(np.int64)
        err[tag] = np.abs(got - bg[on][:, Y0:Y0 + LH, X:X + LW].astype(np.int64)).mean()
    before = np.abs(clip["Y"][on][:, Y0:Y0 + LH, X:X + LW].astype(np.int64) - bg[on][:, Y0:Y0 + LH, X:X + LW]).mean()
    assert err["auto"] <= 1.1 * err["manual"], err
    assert err["auto"] < 0.5 * before, (err, before)


def _worker(rank, world, port, tmpdir, q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    ndev = torch.cuda.device_count()
    devidx = rank % ndev
    torch.cuda.set_device(devidx)
    backend = "nccl" if ndev >= world else "gloo"
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", devidx))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from amatsukaze_amd import Context, DeviceClip
        from amatsukaze_amd import sharding as SH
        dev = torch.device("cuda", devidx)
        ctx = Context(devidx)
        coll = SH.TorchCollectives()
        clip = {k: np.load(os.path.join(tmpdir, f"{k}.npy")) for k in "YUV"}
        a, b = SH.shard_range(N, rank, world)
        loc = DeviceClip(*(torch.from_numpy(np.ascontiguousarray(clip[k][a:b])).to(dev) for k in "YUV"), width=W, height=H)
        lf, cands = SH.find_logo_sharded(ctx, loc, coll)
        S1, SM = lf.sums()
        res = {"rank": rank, "sums": np.concatenate([S1.ravel(), SM.ravel()]).tobytes(), "nframes": lf.nframes,
               "cands": [(c.imgx, c.imgy, c.w, c.h) for c in cands]}
        dst = os.path.join(tmpdir, "sharded.lgd")
        ok, r = SH.scan_logo_auto_sharded(ctx, loc, 1041, dst if rank == 0 else None, 12, 25, coll)
        res["ok"] = ok and coll.error is None
        res["rect"] = (r.imgx, r.imgy, r.w, r.h) if r else None
        q.put(res)
    except Exception as e:        # noqa: BLE001 -- reported to the parent
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc() + str(e)})
    finally:
        dist.destroy_process_group()


def test_sharded_world2_equals_single(gpu, tmp_path):
    import torch.multiprocessing as mp
    from amatsukaze_amd import LogoFinder, ScanLogoAuto
    clip = synth(8)
    for k in "YUV":
        np.save(tmp_path / f"{k}.npy", clip[k])
    single = tmp_path / "single.lgd"
    ok, r = ScanLogoAuto(gpu["ctx"], dclip_of(gpu, clip), 1041, single, 12, 25)
    assert ok
    lf = LogoFinder(gpu["ctx"], W, H, 8)
    lf.add(dclip_of(gpu, clip))
    S1, SM = lf.sums()
    want_sums = np.concatenate([S1.ravel(), SM.ravel()]).tobytes()
    want_cands = [(c.imgx, c.imgy, c.w, c.h) for c in lf.candidates()]
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    procs = [mpc.Process(target=_worker, args=(rk, 2, port, str(tmp_path), q)) for rk in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in procs), key=lambda x: x["rank"])
    for p in procs:
        p.join(timeout=120)
    for x in res:
        assert "error" not in x, x["error"]
        assert x["sums"] == want_sums and x["nframes"] == N
        assert x["cands"] == want_cands
        assert x["ok"] and x["rect"] == (r.imgx, r.imgy, r.w, r.h)
    assert (tmp_path / "sharded.lgd").read_bytes() == single.read_bytes()
    assert all(p.exitcode == 0 for p in procs)
