"""ScanLogo for 9..12-bit clips on the HIP path -- resident, streamed (scan_keep_kernel at 2-byte samples), automatic, from an 'AMTH'
raw clip file and over two sharded ranks: the .lgd is byte for byte the CPU reference's (tests/scanlogo_ref.py, pinned on the CPU by
test_scanlogo_ref_host.py), depth 8 through the new entry points is the existing entry points' bytes, and what must be refused is."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

import scanlogo_hibit_clips as K
from amtlib import Oracle, write_raw_clip
from scanlogo_ref import write_raw_clip_hibit

pytestmark = pytest.mark.gpu

THY, QUOTA, SID = K.THY, K.QUOTA, K.SID
NOMAX = 1 << 30


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return dict(torch=torch, ctx=Context(0), dev=torch.device("cuda:0"))


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def refdir(tmp_path_factory):
    return tmp_path_factory.mktemp("scanlogo_hibit_ref")


def last_error(gpu):
    return gpu["ctx"].lib.amtgpu_last_error(gpu["ctx"].h)


def to_dev(gpu, a, offset=0):
    """the plane in HBM, starting `offset` bytes into its own allocation; 16-bit samples as int16"""
    torch = gpu["torch"]
    a = np.ascontiguousarray(a)
    flat = torch.empty(a.nbytes + offset, dtype=torch.uint8, device=gpu["dev"])
    t = flat[offset:]
    if a.dtype == np.uint16:
        t = t.view(torch.int16)
        a = a.view(np.int16)
    t = t.view(a.shape)
    t.copy_(torch.from_numpy(a))
    return t


def device_clip(gpu, clip, W, H, bits, offset=0):
    from amatsukaze_amd import DeviceClip
    return DeviceClip(*(to_dev(gpu, clip[k], offset) for k in "YUV"), width=W, height=H, bits=bits)


def part(d, a, b):
    from amatsukaze_amd import DeviceClip
    return DeviceClip(d.Y[a:b], d.U[a:b], d.V[a:b], d.width, d.height, d.bits)


def padded(clip, padY, padUV, fill):
    """the same frames in rows padY / padUV samples longer; nothing may read the padding"""
    out = {}
    for k, pad in (("Y", padY), ("U", padUV), ("V", padUV)):
        a = clip[k]
        p = np.full(a.shape[:2] + (a.shape[2] + pad,), fill, a.dtype)
        p[:, :, :a.shape[2]] = a
        out[k] = p
    return out


def cropped(clip, x, y, w, h):
    return {"Y": clip["Y"][:, y:y + h, x:x + w], "U": clip["U"][:, y // 2:(y + h) // 2, x // 2:(x + w) // 2],
            "V": clip["V"][:, y // 2:(y + h) // 2, x // 2:(x + w) // 2]}


def new_stream(gpu, name, bits, quota=QUOTA, rect=None):
    from amatsukaze_amd import ScanLogoStream
    W, H, lw, lh, x, y, _ = K.geometry(name)
    return ScanLogoStream(gpu["ctx"], W, H, *(rect or (x, y, lw, lh)), THY, quota, bits=bits)


def finished(gpu, st, path):
    assert st.finish(SID, path), last_error(gpu)
    return path.read_bytes()


# ---- 1. resident ----
@pytest.mark.parametrize("bits", [10, 12])
def test_resident(gpu, orc, refdir, tmp_path, bits):
    from amatsukaze_amd import ScanLogo
    W, H, lw, lh, x, y, _ = K.geometry("A")
    want, info = K.reference(orc, "A", bits, refdir)
    assert want is not None and (info["kept"], info["nread"]) == (25, 43)
    d = device_clip(gpu, K.clip("A", bits), W, H, bits)
    dst = tmp_path / "resident.lgd"
    calls = []
    assert ScanLogo(gpu["ctx"], d, SID, dst, x, y, lw, lh, THY, QUOTA, cb=lambda p, a, b, c: calls.append(p) or 1), last_error(gpu)
    assert dst.read_bytes() == want
    assert calls and calls[-1] == 1.0


# ---- 2. depth 8 through the new entry points ----
def test_depth_8_through_the_bits_entry_points(gpu, orc, refdir, tmp_path):
    from amatsukaze_amd import binding
    lib, ctx = gpu["ctx"].lib, gpu["ctx"]
    W, H, lw, lh, x, y, n = K.geometry("A")
    d = device_clip(gpu, K.clip("A", 8), W, H, 8)
    yes = binding.CB(lambda *a: 1)
    planes = (C.c_void_p(d.Y.data_ptr()), C.c_void_p(d.U.data_ptr()), C.c_void_p(d.V.data_ptr()), d.strideY, d.strideUV, d.pitchY, d.pitchUV)
    old, new, sold, snew = (tmp_path / f for f in ("old.lgd", "new.lgd", "sold.lgd", "snew.lgd"))
    assert lib.amtgpu_scanlogo(ctx.h, *planes, W, H, n, SID, str(old).encode(), x, y, lw, lh, THY, QUOTA, yes) == 1, last_error(gpu)
    assert lib.amtgpu_scanlogo_bits(ctx.h, *planes, W, H, 8, n, SID, str(new).encode(), x, y, lw, lh, THY, QUOTA, yes) == 1, last_error(gpu)
    assert new.read_bytes() == old.read_bytes()
    status = []
    for create, dst in ((lambda: lib.amtgpu_scanlogo_stream_create(ctx.h, W, H, x, y, lw, lh, THY, QUOTA), sold),
                        (lambda: lib.amtgpu_scanlogo_stream_create_bits(ctx.h, W, H, 8, x, y, lw, lh, THY, QUOTA), snew)):
        h = create()
        assert h, last_error(gpu)
        nk, dn, nr = C.c_int(), C.c_int(), C.c_int64()
        assert lib.amtgpu_scanlogo_stream_feed(h, *planes, n, C.byref(nk), C.byref(dn)) == 1, last_error(gpu)
        assert lib.amtgpu_scanlogo_stream_status(h, C.byref(nr), None, None) == 1
        status.append((nk.value, dn.value, nr.value))
        assert lib.amtgpu_scanlogo_stream_finish(h, SID, str(dst).encode(), yes) == 1, last_error(gpu)
        lib.amtgpu_scanlogo_stream_destroy(h)
    assert status[0] == status[1] == (QUOTA, 1, 43)
    assert snew.read_bytes() == sold.read_bytes() == old.read_bytes()
    assert old.read_bytes() == K.reference(orc, "A", 8, refdir)[0]


# ---- 3. the session at 10 bits ----
def test_session_ragged_batches(gpu, orc, refdir, tmp_path):
    W, H = K.geometry("A")[:2]
    want, info = K.reference(orc, "A", 10, refdir)
    d = device_clip(gpu, K.clip("A", 10), W, H, 10)
    st = new_stream(gpu, "A", 10)
    f0, sizes, seen = 0, (7, 1, 0, 20, 32), []
    for n in sizes:
        nkept, done = st.feed(part(d, f0, f0 + n))
        f0 += n
        seen.append((nkept, done))
    assert [s[1] for s in seen] == [False] * 4 + [True] and sum(sizes[:-1]) < info["nread"] < 60      # the quota closes inside the last batch
    assert all(a[0] <= b[0] for a, b in zip(seen, seen[1:])) and seen[2] == seen[1]
    assert st.status() == {"nread": 43, "nkept": QUOTA, "done": True}
    assert finished(gpu, st, tmp_path / "ragged.lgd") == want


def test_session_one_frame_per_feed_and_a_feed_after_done(gpu, orc, refdir, tmp_path):
    W, H = K.geometry("A")[:2]
    want, info = K.reference(orc, "A", 10, refdir)
    d = device_clip(gpu, K.clip("A", 10), W, H, 10)
    st = new_stream(gpu, "A", 10)
    for i in range(60):
        nkept, done = st.feed(part(d, i, i + 1))
        assert done == (i + 1 >= info["nread"])
    status = st.status()
    assert status == {"nread": 43, "nkept": QUOTA, "done": True}
    assert st.feed(d) == (QUOTA, True) and st.status() == status          # a feed after done changes nothing
    assert finished(gpu, st, tmp_path / "single.lgd") == want


def test_session_feed_rect(gpu, orc, refdir, tmp_path):
    W, H, lw, lh, x, y, _ = K.geometry("A")
    want, _ = K.reference(orc, "A", 10, refdir)
    crop = cropped(K.clip("A", 10), x, y, lw, lh)
    Y, U, V = (to_dev(gpu, crop[k]) for k in "YUV")
    st = new_stream(gpu, "A", 10)
    assert st.feed_rect(Y[:33], U[:33], V[:33])[1] is False
    assert st.feed_rect(Y[33:], U[33:], V[33:]) == (QUOTA, True)
    assert st.status()["nread"] == 43
    assert finished(gpu, st, tmp_path / "rect.lgd") == want


@pytest.mark.parametrize("padY,padUV,offset", [
    (3, 1, 0),        # pitch bytes = 2 mod 4 in both plane kinds: 2-byte lanes; the padding holds a sentinel nothing may read
    (0, 0, 2),        # every plane starts 2 bytes into its allocation
])
def test_session_awkward_addresses(gpu, orc, refdir, tmp_path, padY, padUV, offset):
    W, H = K.geometry("A")[:2]
    want, _ = K.reference(orc, "A", 10, refdir)
    clip = padded(K.clip("A", 10), padY, padUV, 0xA5A5) if padY or padUV else K.clip("A", 10)
    d = device_clip(gpu, clip, W, H, 10, offset)
    assert d.pitchY == W + padY and d.pitchUV == W // 2 + padUV and (d.pitchY * 2) % 4 == (2 if padY else 0)
    assert d.Y.data_ptr() % 16 == offset and d.U.data_ptr() % 16 == offset
    st = new_stream(gpu, "A", 10)
    assert st.feed(part(d, 0, 33))[1] is False
    assert st.feed(part(d, 33, 60)) == (QUOTA, True)
    assert st.status()["nread"] == 43
    assert finished(gpu, st, tmp_path / "awkward.lgd") == want


# ---- 4. odd chroma origin and odd wUV ----
@pytest.mark.parametrize("bits", [10, 12])
def test_odd_chroma_origin_and_width(gpu, orc, refdir, tmp_path, bits):
    from amatsukaze_amd import ScanLogo
    W, H, lw, lh, x, y, _ = K.geometry("odd")
    assert (x // 2) % 2 == 1 and (lw // 2) % 2 == 1
    want, info = K.reference(orc, "odd", bits, refdir)
    assert want is not None and (info["kept"], info["nread"], info["rounds"]) == (25, 43, [3, 10])
    d = device_clip(gpu, K.clip("odd", bits), W, H, bits)
    dst = tmp_path / "resident.lgd"
    assert ScanLogo(gpu["ctx"], d, SID, dst, x, y, lw, lh, THY, QUOTA), last_error(gpu)
    assert dst.read_bytes() == want
    st = new_stream(gpu, "odd", bits)
    assert st.feed(part(d, 0, 33))[1] is False
    assert st.feed(part(d, 33, 60)) == (QUOTA, True)
    assert finished(gpu, st, tmp_path / "session.lgd") == want


# ---- 5. the store grows past its first 256 slots ----
def test_store_grows_at_two_byte_samples(gpu, orc, refdir, tmp_path):
    from amatsukaze_amd import ScanLogo
    W, H, lw, lh, x, y, n = K.geometry("grow")
    want, info = K.reference(orc, "grow", 10, refdir, quota=NOMAX)
    assert want is not None and (info["kept"], info["rounds"]) == (300, [61, 105])
    clip = K.clip("grow", 10)
    crop = cropped(clip, x, y, lw, lh)
    st = new_stream(gpu, "grow", 10, quota=NOMAX)
    nkept = 0
    for f0 in range(0, n, 64):
        nkept, done = st.feed_rect(*(to_dev(gpu, crop[k][f0:f0 + 64]) for k in "YUV"))
        assert not done
    assert nkept == 300 and st.status() == {"nread": n, "nkept": 300, "done": False}
    got = finished(gpu, st, tmp_path / "grown.lgd")
    assert got == want
    dst = tmp_path / "resident.lgd"
    assert ScanLogo(gpu["ctx"], device_clip(gpu, clip, W, H, 10), SID, dst, x, y, lw, lh, THY, NOMAX), last_error(gpu)
    assert dst.read_bytes() == got


# ---- 6. automatic ----
def test_automatic_at_10_bits(gpu, orc, refdir, tmp_path):
    from amatsukaze_amd import DeviceClip, Logo, LogoFinder, ScanLogo, ScanLogoAuto, ScanLogoAutoStream, ScanLogoFileAuto
    W, H, lw, lh, x, y, n = K.geometry("auto")
    clip = K.clip("auto", 10)
    d = device_clip(gpu, clip, W, H, 10)
    lf = LogoFinder(gpu["ctx"], W, H, 10)
    lf.add(d)
    first = lf.candidates(1)[0]
    assert (first.imgx, first.imgy, first.w, first.h) == K.AUTO_RECT
    want, info = K.reference(orc, "auto", 10, refdir, rect=K.AUTO_RECT)
    assert want is not None and (info["kept"], info["nread"], info["rounds"]) == (25, 94, [7, 11])
    auto, manual, streamed, fromfile = (tmp_path / f for f in ("auto.lgd", "manual.lgd", "streamed.lgd", "file.lgd"))
    ok, found = ScanLogoAuto(gpu["ctx"], d, SID, auto, THY, QUOTA)
    assert ok, last_error(gpu)
    assert (found.imgx, found.imgy, found.w, found.h) == K.AUTO_RECT
    assert ScanLogo(gpu["ctx"], d, SID, manual, *K.AUTO_RECT, THY, QUOTA), last_error(gpu)
    assert auto.read_bytes() == manual.read_bytes() == want
    hdr = Logo.load(gpu["ctx"], auto).info
    assert (hdr["imgx"], hdr["imgy"], hdr["w"], hdr["h"], hdr["imgw"], hdr["imgh"]) == K.AUTO_RECT + (W, H)

    def batches():
        for f0 in range(0, n, 50):
            yield DeviceClip(d.Y[f0:f0 + 50], d.U[f0:f0 + 50], d.V[f0:f0 + 50], W, H, 10)

    got = ScanLogoAutoStream(gpu["ctx"], batches, W, H, SID, streamed, THY, QUOTA, bits=10)
    assert (got.imgx, got.imgy, got.w, got.h) == K.AUTO_RECT
    assert streamed.read_bytes() == want
    raw = tmp_path / "clip.amth"
    write_raw_clip_hibit(raw, clip["Y"], clip["U"], clip["V"], W, H, 10)
    ok, found = ScanLogoFileAuto(gpu["ctx"], raw, SID, tmp_path / "work", fromfile, THY, QUOTA)
    assert ok, last_error(gpu)
    assert (found.imgx, found.imgy, found.w, found.h) == K.AUTO_RECT
    assert fromfile.read_bytes() == want


# ---- 7. two ranks ----
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
        from amatsukaze_amd import Context, DeviceClip, ScanLogoStream
        from amatsukaze_amd import sharding as SH
        W, H, lw, lh, x, y, n = K.geometry("A")
        dev = torch.device("cuda", devidx)
        ctx = Context(devidx)
        coll = SH.TorchCollectives()
        clip = {k: np.load(os.path.join(tmpdir, f"{k}.npy")) for k in "YUV"}
        a, b = SH.shard_range(n, rank, world)
        loc = DeviceClip(*(torch.from_numpy(np.ascontiguousarray(clip[k][a:b]).view(np.int16)).to(dev) for k in "YUV"), width=W, height=H,
                         bits=10)
        res = {"rank": rank, "frames": b - a}
        dst = os.path.join(tmpdir, "sharded_resident.lgd")
        ok = SH.scan_logo_sharded(ctx, loc, SID, dst if rank == 0 else None, x, y, lw, lh, THY, QUOTA, coll)
        res["ok_resident"] = bool(ok) and coll.error is None
        res["msg_resident"] = ctx.lib.amtgpu_last_error(ctx.h).decode(errors="replace")
        st = ScanLogoStream(ctx, W, H, x, y, lw, lh, THY, QUOTA, bits=10)
        res["kept"] = st.feed(loc)[0]
        dst = os.path.join(tmpdir, "sharded_stream.lgd")
        ok = SH.scan_logo_stream_finish_sharded(st, SID, dst if rank == 0 else None, coll)
        res["ok_stream"] = bool(ok) and coll.error is None
        res["msg_stream"] = ctx.lib.amtgpu_last_error(ctx.h).decode(errors="replace")
        q.put(res)
    except Exception as e:        # noqa: BLE001 -- reported to the parent, never retried
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc() + str(e)})
    finally:
        dist.destroy_process_group()


def test_two_ranks_at_10_bits(orc, refdir, tmp_path):
    import torch.multiprocessing as mp
    want, info = K.reference(orc, "A", 10, refdir)
    clip = K.clip("A", 10)
    for k in "YUV":
        np.save(tmp_path / f"{k}.npy", clip[k])
    assert 30 < info["nread"]                      # 30 / 30 frames: the quota is filled across the boundary
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    procs = [mpc.Process(target=_worker, args=(rk, 2, port, str(tmp_path), q)) for rk in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda r: r["rank"])
    for p in procs:
        p.join(timeout=120)
    for r in res:
        assert "error" not in r, r["error"]
        assert r["frames"] == 30
        assert r["ok_resident"], r["msg_resident"]
        assert r["ok_stream"], r["msg_stream"]
    assert 0 < res[0]["kept"] < QUOTA
    assert (tmp_path / "sharded_resident.lgd").read_bytes() == want
    assert (tmp_path / "sharded_stream.lgd").read_bytes() == want
    assert all(p.exitcode == 0 for p in procs)


# ---- 8. refusals ----
def test_refusals(gpu, tmp_path):
    from amatsukaze_amd import AmtError, ScanLogoFile, ScanLogoFileAuto, ScanLogoStream, binding
    lib, ctx = gpu["ctx"].lib, gpu["ctx"]
    W, H, lw, lh, x, y, n = K.geometry("A")
    d10 = device_clip(gpu, K.clip("A", 10), W, H, 10)
    d8 = device_clip(gpu, K.clip("A", 8), W, H, 8)
    yes = binding.CB(lambda *a: 1)
    dst = tmp_path / "never.lgd"
    ptrs = [d10.Y.data_ptr(), d10.U.data_ptr(), d10.V.data_ptr()]

    def resident(bits, thy=THY, p=ptrs, strideY=d10.strideY, strideUV=d10.strideUV):
        return lib.amtgpu_scanlogo_bits(ctx.h, *(C.c_void_p(v) for v in p), strideY, strideUV, d10.pitchY, d10.pitchUV, W, H, bits, n, SID,
                                        str(dst).encode(), x, y, lw, lh, thy, QUOTA, yes)

    def auto(bits, p=ptrs, strideY=d10.strideY):
        found = binding.LogoRect()
        return lib.amtgpu_scanlogo_auto_bits(ctx.h, *(C.c_void_p(v) for v in p), strideY, d10.strideUV, d10.pitchY, d10.pitchUV, W, H, bits, n,
                                             SID, str(dst).encode(), THY, QUOTA, yes, None, C.byref(found))

    for bits in (7, 13, 16):
        assert resident(bits) == 0 and b"bits must be 8..12" in last_error(gpu), bits
        assert auto(bits) == 0 and b"bits must be 8..12" in last_error(gpu), bits
        assert not lib.amtgpu_scanlogo_stream_create_bits(ctx.h, W, H, bits, x, y, lw, lh, THY, QUOTA)
        assert b"bits must be 8..12" in last_error(gpu), bits
    assert resident(10, thy=1 << 10) == 0 and b"thy must be below" in last_error(gpu)
    assert not lib.amtgpu_scanlogo_stream_create_bits(ctx.h, W, H, 10, x, y, lw, lh, 1 << 10, QUOTA) and b"thy must be below" in last_error(gpu)
    # an odd byte stride, a plane base at an odd address
    assert resident(10, strideY=d10.strideY + 1) == 0 and b"odd byte stride" in last_error(gpu)
    assert resident(10, strideUV=d10.strideUV + 1) == 0 and b"odd byte stride" in last_error(gpu)
    assert auto(10, strideY=d10.strideY + 1) == 0 and b"odd byte stride" in last_error(gpu)
    for k in range(3):
        p = list(ptrs)
        p[k] += 1
        assert resident(10, p=p) == 0 and b"not aligned to the sample size" in last_error(gpu), k
    assert auto(10, p=[ptrs[0] + 1] + ptrs[1:]) == 0 and b"not aligned to the sample size" in last_error(gpu)
    h = lib.amtgpu_scanlogo_stream_create_bits(ctx.h, W, H, 10, x, y, lw, lh, THY, QUOTA)
    assert h
    feed = lambda p, sy: lib.amtgpu_scanlogo_stream_feed(h, *(C.c_void_p(v) for v in p), sy, d10.strideUV, d10.pitchY, d10.pitchUV, n, None, None)
    assert feed(ptrs, d10.strideY + 1) == 0 and b"odd byte stride" in last_error(gpu)
    assert feed([ptrs[0], ptrs[1] + 1, ptrs[2]], d10.strideY) == 0 and b"not aligned to the sample size" in last_error(gpu)
    nk = C.c_int(-1)
    assert lib.amtgpu_scanlogo_stream_status(h, None, C.byref(nk), None) == 1 and nk.value == 0        # the refused feeds kept nothing
    lib.amtgpu_scanlogo_stream_destroy(h)
    # a clip of another depth than the session's
    with pytest.raises(AmtError, match="10-bit clip fed to a 8-bit session"):
        ScanLogoStream(ctx, W, H, x, y, lw, lh, THY, QUOTA).feed(d10)
    with pytest.raises(AmtError, match="8-bit clip fed to a 10-bit session"):
        ScanLogoStream(ctx, W, H, x, y, lw, lh, THY, QUOTA, bits=10).feed(d8)
    with pytest.raises(AmtError, match="2-byte samples expected"):
        ScanLogoStream(ctx, W, H, x, y, lw, lh, THY, QUOTA, bits=10).feed_rect(d8.Y, d8.U, d8.V)
    # an 'AMTH' header with a depth the format does not carry
    c10 = K.clip("A", 10)
    for bits in (8, 13):
        raw = tmp_path / f"bad{bits}.amth"
        write_raw_clip_hibit(raw, c10["Y"][:2], c10["U"][:2], c10["V"][:2], W, H, bits)
        assert not ScanLogoFile(ctx, raw, SID, tmp_path / "work", dst, x, y, lw, lh, THY, QUOTA)
        assert b"bits must be 9..12" in last_error(gpu), bits
        ok, found = ScanLogoFileAuto(ctx, raw, SID, tmp_path / "work", dst, THY, QUOTA)
        assert not ok and found is None and b"bits must be 9..12" in last_error(gpu), bits
    assert not dst.exists()
    ctx.synchronize()


def test_raw_clip_files_of_both_formats(gpu, orc, refdir, tmp_path):
    """'AMTH' at 10 bits gives the reference's bytes; an 'AMTR' file is read as before"""
    from amatsukaze_amd import ScanLogo, ScanLogoFile
    W, H, lw, lh, x, y, _ = K.geometry("A")
    want, _ = K.reference(orc, "A", 10, refdir)
    c10, c8 = K.clip("A", 10), K.clip("A", 8)
    raw10, raw8, got10, got8, res8 = (tmp_path / f for f in ("a.amth", "a.amtr", "f10.lgd", "f8.lgd", "r8.lgd"))
    write_raw_clip_hibit(raw10, c10["Y"], c10["U"], c10["V"], W, H, 10)
    assert ScanLogoFile(gpu["ctx"], raw10, SID, tmp_path / "work", got10, x, y, lw, lh, THY, QUOTA), last_error(gpu)
    assert got10.read_bytes() == want
    write_raw_clip(raw8, c8["Y"], c8["U"], c8["V"], W, H)
    assert ScanLogoFile(gpu["ctx"], raw8, SID, tmp_path / "work", got8, x, y, lw, lh, THY, QUOTA), last_error(gpu)
    assert ScanLogo(gpu["ctx"], device_clip(gpu, c8, W, H, 8), SID, res8, x, y, lw, lh, THY, QUOTA), last_error(gpu)
    assert got8.read_bytes() == res8.read_bytes() == K.reference(orc, "A", 8, refdir)[0]


# ---- 9. the logo works downstream ----
def test_erase_with_the_10_bit_logo(gpu, tmp_path):
    """frames with the logo fully present, erased (fade 1) with the 10-bit .lgd: mean absolute luma error against the logo-free clip
    below half of what it was (the CPU reference's logo reaches 0.003 x)"""
    from amatsukaze_amd import AMTEraseLogo, Logo, ScanLogo
    W, H, lw, lh, x, y, _ = K.geometry("A")
    clip, bg = K.clip("A", 10), K.clean("A", 10)["Y"]
    on = np.nonzero(K.presence("A") >= 1.0)[0]
    assert len(on) == 31
    dst = tmp_path / "a10.lgd"
    assert ScanLogo(gpu["ctx"], device_clip(gpu, clip, W, H, 10), SID, dst, x, y, lw, lh, THY, QUOTA), last_error(gpu)
    d = device_clip(gpu, {k: clip[k][on] for k in "YUV"}, W, H, 10)
    AMTEraseLogo(gpu["ctx"], Logo.load(gpu["ctx"], dst)).erase(d, np.ones((len(on), 2), np.float32))
    rect = (slice(None), slice(y, y + lh), slice(x, x + lw))
    got = d.Y.cpu().numpy().view(np.uint16)[rect].astype(np.int64)
    want = bg[on][rect].astype(np.int64)
    before = np.abs(clip["Y"][on][rect].astype(np.int64) - want).mean()
    after = np.abs(got - want).mean()
    print(f"mean absolute luma error: {before:.3f} before, {after:.3f} after")
    assert after < 0.5 * before, (after, before)
