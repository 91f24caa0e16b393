"""The streamed ScanLogo session, frame-sharded: two spawned ranks (one device and gloo when the box has a single GPU, as in
test_gpu_sharded.py) each feed their half of the stream into a session of their own; the sharded finish must write the .lgd of ONE
session fed the whole stream -- with a quota that ends inside rank 1's range, and with one rank 0 fills alone (rank 1's share is 0).
A cancelled callback or a spent session on rank 1 ends the finish on BOTH ranks, and the next sharded finish is whole again."""
import os
import socket

import numpy as np
import pytest

import amt_synth as S

pytestmark = pytest.mark.gpu

W, H, LW, LH, X, Y0, N = 352, 240, 96, 48, 224, 18, 60
THY, SID = 12, 1041
QUOTAS = (25, 10)


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
        dev = torch.device("cuda", devidx)
        ctx = Context(devidx)
        coll = SH.TorchCollectives()
        clip = {k: np.load(os.path.join(tmpdir, f"{k}.npy")) for k in "YUV"}
        a, b = SH.shard_range(N, rank, world)
        loc = DeviceClip(*(torch.from_numpy(np.ascontiguousarray(clip[k][a:b])).to(dev) for k in "YUV"), width=W, height=H)
        res = {"rank": rank, "frames": b - a}
        half = (b - a) // 2

        def fed(quota):
            st = ScanLogoStream(ctx, W, H, X, Y0, LW, LH, THY, quota)
            st.feed(DeviceClip(loc.Y[:half], loc.U[:half], loc.V[:half], W, H))
            return st, st.feed(DeviceClip(loc.Y[half:], loc.U[half:], loc.V[half:], W, H))[0]

        def finish(st, tag, cb=None):
            dst = os.path.join(tmpdir, f"sharded_{tag}.lgd")
            ok = SH.scan_logo_stream_finish_sharded(st, SID, dst if rank == 0 else None, coll, cb)
            res[f"ok_{tag}"] = bool(ok) and coll.error is None
            res[f"msg_{tag}"] = ctx.lib.amtgpu_last_error(ctx.h).decode(errors="replace")

        for quota in QUOTAS:
            st, res[f"kept_{quota}"] = fed(quota)
            finish(st, quota)
        # ---- rank 1's callback cancels on its first call: the cancellation rides along the next exchange and BOTH ranks leave with it ----
        calls = []
        finish(fed(25)[0], "cancel", lambda p, nread, total, ngather: (calls.append(p), rank == 0 or len(calls) > 1)[1])
        finish(fed(25)[0], "after_cancel")         # nobody was left out of step: the next sharded finish is whole
        # ---- rank 1 hands in a session it has already finished: its refusal rides along like any other failure ----
        st = fed(25)[0]
        if rank == 1:
            st.finish(SID, os.path.join(tmpdir, "rank1_alone.lgd"))          # (spent whether or not its frames alone make a logo)
        finish(st, "spent")
        finish(fed(25)[0], "after_spent")
        q.put(res)
    except Exception as e:        # noqa: BLE001 -- reported to the parent, never retried
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc() + str(e)})
    finally:
        dist.destroy_process_group()


def test_sharded_finish_equals_one_session(tmp_path):
    import torch
    import torch.multiprocessing as mp
    from amatsukaze_amd import Context, DeviceClip, ScanLogoStream
    _, alpha, alphaUV = S.make_logo(LW, LH)
    clip = S.make_clip_np(N, W, H, 0x5EED0004, alpha, alphaUV, X, Y0, period=20, fade=4, flat_every=2)
    for k in "YUV":
        np.save(tmp_path / f"{k}.npy", clip[k])
    # the single sessions, fed the whole stream
    ctx = Context(0)
    dev = torch.device("cuda:0")
    whole = DeviceClip(*(torch.from_numpy(clip[k]).to(dev) for k in "YUV"), width=W, height=H)
    want, kept_by_rank0 = {}, {}
    for quota in QUOTAS:
        st = ScanLogoStream(ctx, W, H, X, Y0, LW, LH, THY, quota)
        assert st.feed(whole) == (quota, True)
        # where the quota ends: 25 inside rank 1's frames [30, 60), 10 inside rank 0's
        kept_by_rank0[quota] = st.status()["nread"] <= N // 2
        dst = tmp_path / f"single_{quota}.lgd"
        assert st.finish(SID, dst), ctx.lib.amtgpu_last_error(ctx.h)
        want[quota] = dst.read_bytes()
    assert kept_by_rank0 == {25: False, 10: True}
    ctx.synchronize()

    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    procs = [mpc.Process(target=_worker, args=(rk, 2, port, str(tmp_path), q)) for rk in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda x: x["rank"])
    for p in procs:
        p.join(timeout=120)
    for x in res:
        assert "error" not in x, x["error"]
        for quota in QUOTAS:
            assert x[f"ok_{quota}"], x[f"msg_{quota}"]
    for quota in QUOTAS:
        assert (tmp_path / f"sharded_{quota}.lgd").read_bytes() == want[quota], quota
    for x in res:
        assert not x["ok_cancel"] and x["msg_cancel"] == "Cancel requested", x
        assert not x["ok_spent"] and x["ok_after_cancel"] and x["ok_after_spent"], x
    assert "has been finished" in res[1]["msg_spent"] and "another rank failed" in res[0]["msg_spent"], res
    for tag in ("after_cancel", "after_spent"):
        assert (tmp_path / f"sharded_{tag}.lgd").read_bytes() == want[25], tag
    assert res[1]["kept_10"] == 10              # rank 1 kept frames of its own; its share of the quota rank 0 filled is 0
    assert all(p.exitcode == 0 for p in procs)
