"""amtgpu_framestats_sharded_surfaces, world_size 2 (the pattern of tests/test_gpu_sharded.py: one process per rank with its own context; RCCL
with two devices, gloo on one): a P010 clip split at an odd frame, each rank's halo picture passed as `prev`, both ranks get the whole
clip's oracle records; a rank that does not start the clip and brings no `prev` makes both ranks fail together."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, PITCH, H, N, SPLIT, BITS = 37, 48, 21, 9, 5, 10


def _clip():
    import plane_edge_clips as P
    import surface_clips as SC
    rng = np.random.default_rng(90210)
    return P.embed(SC.msb_containers(rng.integers(0, 1 << BITS, (N, H, W)), BITS, rng), PITCH, rows_after=2)


def _worker(rank, world, port, q):
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
        import plane_edge_clips as P
        from amatsukaze_amd import Context, DeviceSurfaces, FrameStats
        from amatsukaze_amd import sharding as SH
        dev = torch.device("cuda", devidx)
        ctx = Context(devidx)
        coll = SH.TorchCollectives()
        clip = _clip()
        f0, f1 = (0, SPLIT) if rank == 0 else (SPLIT, N)
        # this rank's pictures and the one before them, as they lie in its own allocation (poison around every surface)
        h0 = max(0, f0 - 1)
        t = P.to_device(torch, dev, clip.sub(h0, f1 - h0))
        surf = lambda x: DeviceSurfaces(x, None, None, W, H, BITS, interleaved=True, msb=True)
        fs = FrameStats(ctx, W, H, BITS)
        res = {"rank": rank}
        m = SH.framestats_sharded_surfaces(fs, surf(t[f0 - h0:]), f0, N, coll, prev=surf(t[0:1]) if f0 > 0 else None)
        res["metrics"] = m
        try:
            SH.framestats_sharded_surfaces(fs, surf(t[f0 - h0:]), f0, N, coll, prev=None)
            res["halo_required"] = False
        except Exception as e:
            res["halo_required"] = True
            res["halo_msg"] = str(e)
        q.put(res)
    except Exception:      # surface the failure in the parent instead of a bare timeout
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc()})
    finally:
        dist.destroy_process_group()


def test_sharded_surfaces_world2():
    import torch.multiprocessing as mp
    import plane_edge_clips as P
    assert SPLIT % 2 == 1
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    procs = [mpc.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda r: r["rank"])
    for p in procs:
        p.join(timeout=120)
    for r in res:
        assert "error" not in r, r["error"]
    clip = _clip()
    assert clip.form() == "buf_ragged"
    want = P.FS.frame_metrics(clip.frames() >> (16 - BITS))
    for r in res:
        assert np.array_equal(r["metrics"], want), r["rank"]
        assert r["halo_required"]                              # rank 1 lacks its halo: BOTH ranks fail, each with its own message
    assert "needs the picture before it" in res[1]["halo_msg"] and "another rank failed" in res[0]["halo_msg"]
    assert all(p.exitcode == 0 for p in procs)
