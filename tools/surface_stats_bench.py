#!/usr/bin/env python3
"""What the frame metrics cost straight from P010 decoder surfaces (profiles/surface_stats.json).  HIP events on the context's stream around
--inner back-to-back calls, median and min-max of --reps repetitions (at least 5) after a warm-up round; the routes that are compared
alternate in this one process.

Shapes: 1920x1080 and 1440x1080 P010 (10-bit MSB, random non-zero low bits under every sample), batches of 64 pictures.

  a  run_device_surfaces on the P010 surfaces: frame_stats_kernel's MSB form reads the Y containers and shifts them in registers.
  b  the only route the parent commit offers from the same surfaces: weave_fields(nv12=True, msb=True) of the whole pictures into a planar
     LSB clip, then run_device on its Y planes.
  c  run_device on an already planar LSB copy of the same pictures: the plain 16-bit kernel, the same algorithmic bytes as a.

The three records must be byte-equal.  a against c is the cost of the packed shifts; a's Y bytes per second are given as a fraction of
HBM peak.

    python tools/surface_stats_bench.py --out profiles/surface_stats.json [--reps 7] [--inner 10]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

BATCH, BITS = 64, 10
HBM_PEAK_GBS = 8000.0                  # as bench.py
SHAPES = (dict(name="1920x1080 P010 (10-bit MSB)", W=1920, H=1080), dict(name="1440x1080 P010 (10-bit MSB)", W=1440, H=1080))


def spread(xs, unit="us", digits=2):
    return {f"median_{unit}": round(statistics.median(xs), digits), f"min_{unit}": round(min(xs), digits), f"max_{unit}": round(max(xs), digits),
            unit: [round(x, digits) for x in xs]}


def timed_us(torch, fn, inner):
    """microseconds per call of `inner` back-to-back calls between two HIP events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / inner


def alternate(torch, routes, reps, inner):
    times = {k: [] for k in routes}
    for rep in range(reps + 1):                               # (the first round warms up)
        for name, fn in routes.items():
            us = timed_us(torch, fn, inner)
            if rep:
                times[name].append(us)
    return times


def bench_shape(ctx, torch, sh, reps, inner):
    from amatsukaze_amd import DeviceClip, DeviceSurfaces, FrameStats, weave_fields
    dev = torch.device("cuda:0")
    W, H, s = sh["W"], sh["H"], 16 - BITS
    g = torch.Generator(device=dev).manual_seed(0x57A7 + W)

    def samples(shape):
        return torch.randint(0, 1 << BITS, shape, generator=g, device=dev, dtype=torch.int64)

    def containers(v):
        v = (v << s) | torch.randint(1, 1 << s, v.shape, generator=g, device=dev, dtype=torch.int64)
        return torch.where(v >= 32768, v - 65536, v).to(torch.int16)         # the uint16 container's bits in an int16

    y = samples((BATCH, H, W))
    planarY = y.to(torch.int16)                                                                    # c: a planar copy of the same pictures
    surf = DeviceSurfaces(containers(y), containers(samples((BATCH, H // 2, W))), None, W, H, BITS, True, True)
    del y
    woven = DeviceClip(torch.empty((BATCH, H, W), dtype=torch.int16, device=dev), torch.empty((BATCH, H // 2, W // 2), dtype=torch.int16, device=dev),
                       torch.empty((BATCH, H // 2, W // 2), dtype=torch.int16, device=dev), W, H, BITS)
    fs = FrameStats(ctx, W, H, BITS)
    out = {k: torch.zeros((BATCH, 8), dtype=torch.int64, device=dev) for k in "abc"}
    torch.cuda.synchronize()

    def route_b():
        weave_fields(ctx, surf.Y, surf.U, None, woven, None, None, nv12=True, msb=True)
        fs.run_device(woven.Y, out["b"])

    names = {"a": "a_run_device_surfaces_on_p010", "b": "b_weave_whole_pictures_then_run_device", "c": "c_run_device_on_a_planar_lsb_copy"}
    t = alternate(torch, {names["a"]: lambda: fs.run_device_surfaces(surf, out["a"]), names["b"]: route_b,
                          names["c"]: lambda: fs.run_device(planarY, out["c"])}, reps, inner)
    torch.cuda.synchronize()
    equal = bool(torch.equal(out["a"], out["b"]) and torch.equal(out["a"], out["c"]))
    assert equal, "the three routes' records differ"
    res = {"shape": sh["name"], "batch": BATCH, "records_byte_equal": equal}
    for k, xs in t.items():
        res[k] = spread(xs)
    a, b, c = (res[names[k]] for k in "abc")
    y_bytes = W * H * 2 * BATCH
    gbs = y_bytes / (a["median_us"] * 1e-6) / 1e9
    res["y_bytes_per_call"] = y_bytes
    res["a_achieved_gbs"] = round(gbs, 1)
    res["a_frac_hbm_peak"] = round(gbs / HBM_PEAK_GBS, 4)
    res["hbm_peak_gbs"] = HBM_PEAK_GBS
    res["a_below_b"] = bool(a["max_us"] < b["min_us"])
    res["ratio_b_over_a"] = round(b["median_us"] / a["median_us"], 2)
    allowed = max(0.05 * c["median_us"], a["max_us"] - a["min_us"], c["max_us"] - c["min_us"])
    res["a_vs_c"] = {"a_median_minus_c_median_us": round(a["median_us"] - c["median_us"], 2), "ratio_a_over_c": round(a["median_us"] / c["median_us"], 4),
                     "allowed_us": round(allowed, 2), "allowed_is": "the larger of 5 % of c and the two routes' own min-max spreads",
                     "within": bool(abs(a["median_us"] - c["median_us"]) <= allowed)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_stats.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    reps, inner = max(5, a.reps), max(1, a.inner)
    import torch
    from amatsukaze_amd import Context
    ctx = Context(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "inner": inner,
           "timing": "HIP events on the context's stream around `inner` back-to-back calls, microseconds per call of 64 pictures; median and "
                     "min-max of the repetitions after one warm-up round; the routes of a shape alternate in one process",
           "shapes": []}
    for sh in SHAPES:
        res["shapes"].append(bench_shape(ctx, torch, sh, reps, inner))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
