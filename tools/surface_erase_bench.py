#!/usr/bin/env python3
"""What erasing and analysing decoder surfaces where they lie costs (profiles/surface_erase.json).  HIP events on the context's stream
around --inner back-to-back calls, median and min-max of --reps repetitions (at least 5) after a warm-up round; the routes that are
compared alternate in this one process.

Shapes: 1440x1080 NV12 with the logo at (1120, 64), and 1920x1080 P010 (10-bit MSB) with the logo at (1600, 64); a 256x128 logo, batches of
64 frames, all fades {1, 1} so that every rectangle is rewritten.

  a  erase_surfaces(d_fades) in place on the surfaces.
  b  the only route the parent commit offers from the same surfaces: weave_fields(nv12=True[, msb=True]) of the whole frames into a planar
     clip, then erase_device_fades on it.  It ENDS IN PLANAR FRAMES, not in surfaces: an encoder host would still have to write the
     result back into a surface itself, so this understates what the old route costs it.
  c  erase_device_fades on a planar copy of the same pictures: the same algorithmic bytes as a.

a's rectangle bytes (read + written, the way bench.py's roofline counts delogo_kernel's) per second are given as a fraction of HBM peak.
Also: analyze_surfaces on the P010 batch against weave + analyze_device; the records must be equal.

    python tools/surface_erase_bench.py --out profiles/surface_erase.json [--reps 7] [--inner 20]
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

LW, LH, BATCH = 256, 128, 64
HBM_PEAK_GBS = 8000.0                  # as bench.py
SHAPES = (dict(name="1440x1080 NV12", W=1440, H=1080, X=1120, Y0=64, bits=8, msb=False),
          dict(name="1920x1080 P010 (10-bit MSB)", W=1920, H=1080, X=1600, Y0=64, bits=10, msb=True))


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
    import amt_synth as S
    from amatsukaze_amd import AMTAnalyzeLogo, AMTEraseLogo, DeviceClip, DeviceSurfaces, Logo, weave_fields
    dev = torch.device("cuda:0")
    W, H, X, Y0, bits, msb = sh["W"], sh["H"], sh["X"], sh["Y0"], sh["bits"], sh["msb"]
    es = 1 if bits <= 8 else 2
    tdt = torch.uint8 if bits <= 8 else torch.int16
    g = torch.Generator(device=dev).manual_seed(0x5E + bits)

    def samples(shape):
        return torch.randint(0, 1 << bits, shape, generator=g, device=dev, dtype=torch.int64)

    def containers(v):
        if msb:
            s = 16 - bits
            v = (v << s) | torch.randint(1, 1 << s, v.shape, generator=g, device=dev, dtype=torch.int64)
            v = torch.where(v >= 32768, v - 65536, v)         # the uint16 container's bits in an int16
        return v.to(tdt)

    y, u, v = samples((BATCH, H, W)), samples((BATCH, H // 2, W // 2)), samples((BATCH, H // 2, W // 2))
    planar = DeviceClip(y.to(tdt), u.to(tdt), v.to(tdt), W, H, bits)                               # c: a planar copy of the same pictures
    surf = DeviceSurfaces(containers(y), containers(torch.stack((u, v), dim=-1).reshape(BATCH, H // 2, W)).contiguous(), None, W, H, bits, True, msb)
    del y, u, v
    woven = DeviceClip(torch.empty((BATCH, H, W), dtype=tdt, device=dev), torch.empty((BATCH, H // 2, W // 2), dtype=tdt, device=dev),
                       torch.empty((BATCH, H // 2, W // 2), dtype=tdt, device=dev), W, H, bits)
    data = S.make_logo(LW, LH)[0]
    logo = Logo.from_planes(ctx, data, LW, LH, W, H, X, Y0)
    er = AMTEraseLogo(ctx, logo)
    d_fades = torch.ones((BATCH, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    # the analysis first, while the surfaces still hold the pictures the planar copy holds
    res = {"shape": sh["name"], "logo": [X, Y0, LW, LH], "batch": BATCH, "fades": "{1, 1} for every frame"}
    if msb:
        an = AMTAnalyzeLogo(ctx, logo, 0.35)
        rec_s = torch.empty((BATCH, 33), dtype=torch.float32, device=dev)
        rec_w = torch.empty_like(rec_s)

        def weave_then_analyze():
            weave_fields(ctx, surf.Y, surf.U, None, woven, None, None, nv12=True, msb=True)
            an.analyze_device(woven.Y, bits, rec_w)

        t = alternate(torch, {"analyze_surfaces": lambda: an.analyze_surfaces(surf, rec_s), "weave_then_analyze_device": weave_then_analyze}, reps, inner)
        torch.cuda.synchronize()
        equal = bool(torch.equal(rec_s, rec_w))
        assert equal, "analyze_surfaces and weave + analyze_device disagree"
        res["analyze"] = {"analyze_surfaces": spread(t["analyze_surfaces"]), "weave_then_analyze_device": spread(t["weave_then_analyze_device"]),
                          "records_equal": equal,
                          "ratio_weave_over_surfaces": round(statistics.median(t["weave_then_analyze_device"]) / statistics.median(t["analyze_surfaces"]), 2)}

    def route_b():
        weave_fields(ctx, surf.Y, surf.U, None, woven, None, None, nv12=True, msb=msb)
        er.erase_device_fades(woven, d_fades)

    t = alternate(torch, {"a_erase_surfaces_in_place": lambda: er.erase_surfaces(surf, d_fades=d_fades),
                          "b_weave_whole_frames_then_erase_device_fades": route_b,
                          "c_erase_device_fades_on_a_planar_copy": lambda: er.erase_device_fades(planar, d_fades)}, reps, inner)
    for k, xs in t.items():
        res[k] = spread(xs)
    a, c = res["a_erase_surfaces_in_place"], res["c_erase_device_fades_on_a_planar_copy"]
    rect_bytes = 2 * (LW * LH + 2 * (LW // 2) * (LH // 2)) * es * BATCH                             # read + written, as bench.py counts delogo_kernel
    gbs = rect_bytes / (a["median_us"] * 1e-6) / 1e9
    res["a_rectangle_bytes_per_call"] = rect_bytes
    res["a_achieved_gbs"] = round(gbs, 1)
    res["a_frac_hbm_peak"] = round(gbs / HBM_PEAK_GBS, 4)
    res["hbm_peak_gbs"] = HBM_PEAK_GBS
    res["b_note"] = ("b ends in planar frames, not in surfaces: it understates what the old route costs an encoder host, which must still write "
                     "the result back into a surface")
    res["b_bytes_woven_per_call"] = 2 * (W * H * 3 // 2) * es * BATCH
    res["ratio_b_over_a"] = round(res["b_weave_whole_frames_then_erase_device_fades"]["median_us"] / a["median_us"], 2)
    c_spread = c["max_us"] - c["min_us"]
    res["a_vs_c"] = {"a_median_minus_c_median_us": round(a["median_us"] - c["median_us"], 2), "c_max_minus_min_us": round(c_spread, 2),
                     "a_exceeds_c_by_more_than_c_spread": bool(a["median_us"] - c["median_us"] > c_spread)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_erase.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    reps, inner = max(5, a.reps), max(1, a.inner)
    import torch
    from amatsukaze_amd import Context
    ctx = Context(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "inner": inner,
           "timing": "HIP events on the context's stream around `inner` back-to-back calls, microseconds per call; median and min-max of the "
                     "repetitions after one warm-up round; the routes of a shape alternate in one process",
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
