"""Times the logo finder's detection kernel (logofind_kernels.hip) with HIP events over 10 000 frames resident in HBM, at 1440 x 1080
8-bit and 1920 x 1080 10-bit, and writes profiles/logofind.json: ms per 10 000 frames, the algorithmic bytes (W * H * sample size
per frame) per second and their fraction of the 8 TB/s HBM peak.

    python tools/logofind_bench.py [--frames 10000] [--reps 5] [--out profiles/logofind.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def run(ctx, torch, W, H, bits, frames, reps):
    from amatsukaze_amd import LogoFinder
    es = 1 if bits <= 8 else 2
    dt = torch.uint8 if es == 1 else torch.int16
    Y = torch.empty((frames, H, W), dtype=dt, device="cuda:0")
    g = torch.Generator(device="cuda:0").manual_seed(1234)
    for a in range(0, frames, 1000):       # (in slices: randint materialises int64 temporaries)
        Y[a:a + 1000] = torch.randint(0, 1 << bits, (min(1000, frames - a), H, W), generator=g, device="cuda:0", dtype=torch.int64).to(dt)
    lf = LogoFinder(ctx, W, H, bits)
    lf.add_device(Y)                       # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        lf.add_device(Y)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    del Y
    torch.cuda.empty_cache()
    best = min(ms)
    nbytes = W * H * es * frames
    return {"width": W, "height": H, "bits": bits, "frames": frames, "reps": reps, "ms": [round(x, 4) for x in ms],
            "ms_per_10k_frames": round(best * 10000 / frames, 4), "median_ms_per_10k_frames": round(sorted(ms)[len(ms) // 2] * 10000 / frames, 4),
            "algorithmic_GBps": round(nbytes / (best * 1e-3) / 1e9, 1), "fraction_of_hbm_peak": round(nbytes / (best * 1e-3) / HBM_PEAK, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logofind.json"))
    args = ap.parse_args()
    import torch
    from amatsukaze_amd import Context
    ctx = Context(0)
    res = {"kernel": "logofind_kernel", "timing": "HIP events around amtgpu_logofind_add_batch, best of reps after one warm-up",
           "hbm_peak_Bps": HBM_PEAK, "device": torch.cuda.get_device_name(0),
           "cases": [run(ctx, torch, 1440, 1080, 8, args.frames, args.reps), run(ctx, torch, 1920, 1080, 10, args.frames, args.reps)]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
