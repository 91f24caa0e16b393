"""The audio level pass (AudioLevels, csrc/audio_kernels.hip) measured on an MI355X; writes profiles/audio_levels.json.

  kernel   audio_levels_kernel alone on PCM resident in HBM, 48 kHz stereo under 30000/1001 video, for 10 000 video frames (64 MB) and
           431 568 (a 4-hour stream, 2.76 GB): HIP events around one launch, median [min - max] of 7 after 2 warm-up launches.  The
           64 MB case walks through a ring of distinct buffers of 1 GiB in all, so that no launch finds its input in the 256 MB
           Infinity Cache left by the one before.  Rate = bytes of PCM read / time, also as a fraction of 8 TB/s.
  amts     AudioLevels.run_amts on a generated 10 000-frame wave file, host clock around the synchronous call, median [min - max] of 7
           after one warm-up, as video frames per second.  The file has just been written: it is read from the page cache, not a disk.

    python tools/audio_levels_bench.py [--out profiles/audio_levels.json] [--frames 10000,431568]
There is no CPU path: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RATE, CH, FPS = 48000, 2, (30000, 1001)
HBM_BYTES_PER_S = 8e12
REPS, WARMUP = 7, 2


def b(n):
    return n * RATE * FPS[1] // FPS[0]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def kernel_case(A, ctx, torch, np, nframes):
    ns = b(nframes)
    nbytes = ns * CH * 2
    nbuf = max(1, min(16, -(-(1 << 30) // nbytes))) if nbytes < (1 << 30) else 1
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234 + nframes)
    bufs = [torch.randint(-32768, 32768, (ns * CH,), dtype=torch.int16, device="cuda", generator=gen) for _ in range(nbuf)]
    al = A.AudioLevels(ctx, RATE, CH, *FPS, ns)
    out = torch.zeros((nframes, 4), dtype=torch.int64, device="cuda")
    # the records of 64 frames spread over the stream against numpy, before any timing
    al.run_device(bufs[0], 0, 0, nframes, out=out)
    ctx.synchronize()
    got = out.cpu().numpy().astype(np.uint64)
    for f in np.linspace(0, nframes - 1, 64).astype(np.int64):
        x = np.abs(bufs[0][b(int(f)) * CH:b(int(f) + 1) * CH].cpu().numpy().astype(np.int64))
        want = (int(x.max()), int(x.sum()), int((x * x).sum()), x.size)
        assert tuple(int(v) for v in got[f]) == want, (int(f), got[f], want)
    assert int(got[:, 3].sum()) == ns * CH
    ms = []
    for i in range(WARMUP + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        al.run_device(bufs[i % nbuf], 0, 0, nframes, out=out)
        e1.record()
        e1.synchronize()
        if i >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    t = spread(ms)
    rate = nbytes / (t["median"] * 1e-3)
    return {"frames": nframes, "sample_frames": ns, "pcm_bytes": nbytes, "distinct_buffers": nbuf, "ms": t, "bytes_per_s": rate,
            "fraction_of_8TBps": rate / HBM_BYTES_PER_S, "checked_frames_against_numpy": 64}


def amts_case(A, ctx, np, nframes):
    from amts_util import write_amts
    spf = 1024
    naudio = -(-b(nframes) // spf)
    rng = np.random.default_rng(99)
    pcm = rng.integers(-32768, 32768, (naudio * spf, 2)).astype(np.int16)
    with tempfile.TemporaryDirectory() as d:
        wav, dat = os.path.join(d, "bench.wav"), os.path.join(d, "bench.dat")
        with open(wav, "wb") as f:
            f.write(b"\0" * 44 + pcm.tobytes())
        vfmt = (0, 1440, 1080, 1440, 1080, 4, 3, 30000, 1001, 1, 1, 1, False, True)
        write_amts(dat, "bench.ts", wav, vfmt, (2, RATE), [], [(k, 44 + k * spf * 4, spf * 4) for k in range(naudio)])
        amts = A.AmtsFile(dat, ctx)
        al = A.AudioLevels(ctx, RATE, CH, *FPS, amts.audio_info()[1])
        n = al.num_frames()
        secs = []
        for i in range(1 + REPS):
            t0 = time.perf_counter()
            got = al.run_amts(amts)
            t1 = time.perf_counter()
            if i:
                secs.append(t1 - t0)
        assert np.array_equal(got, al.run(pcm))                    # the same records as the kernel on the samples themselves
    t = spread(secs)
    return {"frames": n, "wave_bytes": int(pcm.nbytes), "file": "just written: page cache, no disk", "seconds": t, "frames_per_s": n / t["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_levels.json"))
    ap.add_argument("--frames", default="10000,431568")
    ap.add_argument("--amts-frames", type=int, default=10000)
    args = ap.parse_args()
    import numpy as np
    import torch
    import amatsukaze_amd as A
    ctx = A.Context(0)
    res = {"what": "audio_levels_kernel on resident PCM (HIP events, median [min - max] of %d after %d warm-up launches) and AudioLevels.run_amts "
                   "(host clock); 48 kHz stereo int16 under 30000/1001 video" % (REPS, WARMUP),
           "device": torch.cuda.get_device_name(0), "kernel": [], "amts": None}
    for n in [int(v) for v in args.frames.split(",") if v]:
        res["kernel"].append(kernel_case(A, ctx, torch, np, n))
        print(json.dumps(res["kernel"][-1]), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    res["amts"] = amts_case(A, ctx, np, args.amts_frames)
    print(json.dumps(res["amts"]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
