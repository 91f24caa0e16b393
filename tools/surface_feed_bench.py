#!/usr/bin/env python3
"""What feeding decoder surfaces buys and what it costs the planar paths (profiles/surface_feed.json).  HIP events on the context's stream,
median and min-max of --reps repetitions (at least 5) after a warm-up; libraries that are compared alternate in this one process.

  1. feed      1440x1080 NV12 8-bit, rectangle 256x128 at (1120, 64), 4 batches of 64 frames (one frame in four flat-bordered, no quota):
               ScanLogoStream.feed_surfaces against the only route without it -- weave_fields(nv12=True) into a planar clip, then feed.
               Events around the four batches of a fresh session; both routes' .lgd must be the same file.  The two copy kernels alone
               (surfaces_extract_kernel, weave_fields_kernel) come from a profiled pass of their own (the context's event spans).
  2. finder    1920x1080 10-bit, 10 000 frames resident: amtgpu_logofind_add_batch of --parent (a libamt_gpu.so of the parent commit) against
               this tree's, alternated; "the LSB finder must not pay": change's median <= parent's median + parent's (max - min).
               Needed because logofind_kernels.hip now takes its kernel from logofind_body.h.
               (The 8-bit ScanLogo session under the same rule is tools/scanlogo_hibit_bench.py --time OUT --parent LIB, run as it is;
               --merge puts its result into the output of this tool.)
  3. msb       the same frames MSB-aligned with random low bits: amtgpu_logofind_add_surfaces against add_batch on the LSB frames,
               alternated; the ratio of the medians, and that both leave the same sums.

    python tools/surface_feed_bench.py --out profiles/surface_feed.json [--reps 7] [--parent LIB] [--frames 10000] [--merge HIBIT.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, H, LW, LH, X, Y0, SEED = 1440, 1080, 256, 128, 1120, 64, 0x5EED00C3
FRAMES, BATCH, FLAT, THY, NOMAX = 256, 64, 4, 12, 1 << 30
FW, FH, FBITS = 1920, 1080, 10


def spread(xs, unit="ms", digits=4):
    return {f"median_{unit}": round(statistics.median(xs), digits), f"min_{unit}": round(min(xs), digits), f"max_{unit}": round(max(xs), digits),
            unit: [round(x, digits) for x in xs]}


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


# ---- 1. feed_surfaces against weave + feed ----
def bench_feed(ctx, torch, reps, tmp):
    import amt_synth as S
    from amatsukaze_amd import DeviceClip, DeviceSurfaces, ScanLogoStream, weave_fields
    dev = torch.device("cuda:0")
    _, alpha, alphaUV = S.make_logo(LW, LH)
    c = S.make_clip_torch(FRAMES, W, H, SEED, alpha, alphaUV, X, Y0, dev, bits=8, period=900, fade=12, flat_every=FLAT)
    UV = torch.stack((c["U"], c["V"]), dim=-1).reshape(FRAMES, H // 2, W).contiguous()          # U0 V0 U1 V1 ...
    Y = c["Y"]
    del c
    planar = DeviceClip(torch.empty((BATCH, H, W), dtype=torch.uint8, device=dev), torch.empty((BATCH, H // 2, W // 2), dtype=torch.uint8, device=dev),
                        torch.empty((BATCH, H // 2, W // 2), dtype=torch.uint8, device=dev), W, H, 8)
    torch.cuda.synchronize()
    batches = [(f0, min(FRAMES, f0 + BATCH)) for f0 in range(0, FRAMES, BATCH)]

    def surfaces_route(st):
        for a, b in batches:
            st.feed_surfaces(DeviceSurfaces(Y[a:b], UV[a:b], None, W, H, 8, True, False))

    def weave_route(st):
        for a, b in batches:
            weave_fields(ctx, Y[a:b], UV[a:b], None, planar, None, None, nv12=True)
            st.feed(planar)

    routes = {"feed_surfaces": surfaces_route, "weave_then_feed": weave_route}
    times, sha, kept = {k: [] for k in routes}, {}, {}
    for rep in range(reps + 1):                           # (the first round warms up)
        for name, route in routes.items():                # alternated
            st = ScanLogoStream(ctx, W, H, X, Y0, LW, LH, THY, NOMAX)
            ms = timed(torch, lambda: route(st))
            if rep:
                times[name].append(ms)
            kept[name] = st.status()["nkept"]
            if rep == reps:
                ctx.check(st.finish(1041, tmp), "finish")
                sha[name] = hashlib.sha256(open(tmp, "rb").read()).hexdigest()
                os.remove(tmp)
    # the copy kernels alone: the context's event spans over one more round
    ctx.profile(True)
    for route in routes.values():
        route(ScanLogoStream(ctx, W, H, X, Y0, LW, LH, THY, NOMAX))
    ctx.synchronize()
    prof = ctx.profile_report()
    ctx.profile(False)
    nb = len(batches)
    res = {"shape": f"{W}x{H} NV12 8-bit", "rect": [X, Y0, LW, LH], "frames": FRAMES, "batch": BATCH, "flat_every": FLAT, "kept": kept,
           "clock": "HIP events around the %d feeds of a fresh session (each feed reads its verdicts back)" % nb,
           "lgd_equal": sha["feed_surfaces"] == sha["weave_then_feed"], "lgd_sha256": sha["feed_surfaces"]}
    for name in routes:
        res[name] = spread(times[name])
        res[name]["median_ms_per_batch"] = round(res[name]["median_ms"] / nb, 4)
    res["ratio_weave_over_surfaces"] = round(res["weave_then_feed"]["median_ms"] / res["feed_surfaces"]["median_ms"], 2)
    res["copy_kernels_alone"] = {k: {"calls": v[0], "mean_us": round(1000.0 * v[1] / max(1, v[0]), 2)} for k, v in prof.items()
                                 if k in ("surfaces_extract_kernel", "weave_fields_kernel")}
    res["bytes_per_frame"] = {"extract_in": LW * LH * 3 // 2, "extract_out": LW * LH * 3 // 2, "weave_in_plus_out": 2 * W * H * 3 // 2,
                              "note": "the extraction reads 1.5 * w * h NV12 bytes and writes as many planar ones"}
    return res


# ---- 2. / 3. the finder ----
def raw_lib(path):
    lib = C.CDLL(path)
    p, i, i64, s = C.c_void_p, C.c_int, C.c_int64, C.c_char_p
    for name, (res, args) in {"amtgpu_context_create": (p, [i]), "amtgpu_context_set_stream": (i, [p, p]), "amtgpu_last_error": (s, [p]),
                              "amtgpu_logofind_create": (p, [p, i, i, i]), "amtgpu_logofind_destroy": (None, [p]),
                              "amtgpu_logofind_add_batch": (i, [p, p, i64, i, i]), "amtgpu_logofind_add_surfaces": (i, [p, p, i]),
                              "amtgpu_logofind_get_sums": (i, [p, p])}.items():
        f = getattr(lib, name, None)
        if f is not None:
            f.restype, f.argtypes = res, args
    ctx = lib.amtgpu_context_create(0)
    lib.amtgpu_context_set_stream(ctx, C.c_void_p(1))          # torch's stream (the legacy default one): the events below are recorded on it
    return lib, ctx


def bench_finder(torch, reps, frames, parent):
    import numpy as np
    from amatsukaze_amd import binding
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1234)
    Yl = torch.empty((frames, FH, FW), dtype=torch.int16, device=dev)
    Ym = torch.empty((frames, FH, FW), dtype=torch.int16, device=dev)
    sh = 16 - FBITS
    for a in range(0, frames, 500):        # (in slices: randint materialises int64 temporaries)
        n = min(500, frames - a)
        v = torch.randint(0, 1 << FBITS, (n, FH, FW), generator=g, device=dev, dtype=torch.int64)
        Yl[a:a + n] = v.to(torch.int16)
        m = (v << sh) | torch.randint(1, 1 << sh, (n, FH, FW), generator=g, device=dev, dtype=torch.int64)
        Ym[a:a + n] = torch.where(m >= 32768, m - 65536, m).to(torch.int16)          # the uint16 container's bits in an int16
        del v, m
    torch.cuda.synchronize()
    change = raw_lib(os.path.join(ROOT, "amatsukaze_amd", "libamt_gpu.so"))
    libs = {"change": change}
    if parent:
        libs = {"parent": raw_lib(parent), "change": change}
    stride = FW * FH * 2

    def finder(lib, ctx):
        h = lib.amtgpu_logofind_create(ctx, FW, FH, FBITS)
        if not h:
            raise RuntimeError(lib.amtgpu_last_error(ctx).decode(errors="replace"))
        return h

    def add_lsb(lib, h):
        if not lib.amtgpu_logofind_add_batch(h, C.c_void_p(Yl.data_ptr()), stride, FW, frames):
            raise RuntimeError("add_batch failed")

    desc = binding.Surfaces(C.c_void_p(Ym.data_ptr()), None, None, stride, 0, FW, 0, FBITS, 1, 1, 0)

    def add_msb(lib, h):
        if not lib.amtgpu_logofind_add_surfaces(h, C.byref(desc), frames):
            raise RuntimeError("add_surfaces failed")

    def sums(lib, h):
        s = np.zeros(2 * FW * FH, np.int64)
        lib.amtgpu_logofind_get_sums(h, s.ctypes.data_as(C.c_void_p))
        return hashlib.sha256(s.tobytes()).hexdigest()

    # 2. parent against change, LSB
    hs = {k: finder(*v) for k, v in libs.items()}
    t = {k: [] for k in libs}
    for rep in range(reps + 1):
        for k, (lib, ctx) in libs.items():
            ms = timed(torch, lambda: add_lsb(lib, hs[k]))
            if rep:
                t[k].append(ms * 10000.0 / frames)
    res = {"shape": f"{FW}x{FH} {FBITS}-bit", "frames": frames, "clock": "HIP events around one amtgpu_logofind_add_batch, ms per 10 000 frames"}
    lsb = {"change": spread(t["change"])}
    if parent:
        p = lsb["parent"] = spread(t["parent"])
        allowed = p["median_ms"] + (p["max_ms"] - p["min_ms"])
        lsb["sums_equal_parent"] = sums(libs["parent"][0], hs["parent"]) == sums(change[0], hs["change"])
        lsb["lsb_finder_must_not_pay"] = {"rule": "change median <= parent median + (parent max - parent min)", "allowed_ms": round(allowed, 4),
                                          "holds": lsb["change"]["median_ms"] <= allowed}
    for k, (lib, _) in libs.items():
        lib.amtgpu_logofind_destroy(hs[k])
    res["lsb_parent_vs_change"] = lsb
    # 3. MSB against LSB on this tree's library
    lib, ctx = change
    hl, hm = finder(lib, ctx), finder(lib, ctx)
    t = {"lsb": [], "msb": []}
    for rep in range(reps + 1):
        for k, fn, h in (("lsb", add_lsb, hl), ("msb", add_msb, hm)):
            ms = timed(torch, lambda: fn(lib, h))
            if rep:
                t[k].append(ms * 10000.0 / frames)
    res["msb_vs_lsb"] = {"lsb_add_batch": spread(t["lsb"]), "msb_add_surfaces": spread(t["msb"]),
                         "ratio_msb_over_lsb": round(statistics.median(t["msb"]) / statistics.median(t["lsb"]), 4),
                         "sums_equal": sums(lib, hl) == sums(lib, hm)}
    lib.amtgpu_logofind_destroy(hl)
    lib.amtgpu_logofind_destroy(hm)
    del Yl, Ym
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_feed.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--parent")
    ap.add_argument("--merge", help="a result of tools/scanlogo_hibit_bench.py --time --parent: its 8-bit block goes into the output")
    ap.add_argument("--only", choices=("feed", "finder"))
    a = ap.parse_args()
    reps = max(5, a.reps)
    import torch
    from amatsukaze_amd import Context
    ctx = Context(0)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.update({"device": torch.cuda.get_device_name(0), "timing": "HIP events, median and min-max of the repetitions after one warm-up round",
                "reps": reps})
    if a.only != "finder":
        res["1_feed_surfaces_vs_weave_then_feed"] = bench_feed(ctx, torch, reps, a.out + ".lgd")
        torch.cuda.empty_cache()
    if a.only != "feed":
        res["2_3_logo_finder"] = bench_finder(torch, reps, a.frames, a.parent)
    if a.merge:
        m = json.load(open(a.merge))
        res["2_scanlogo_session_8bit_parent_vs_change"] = {"tool": "tools/scanlogo_hibit_bench.py --time --parent, as it is",
                                                           "clock": m.get("clock"), "reps": m.get("reps"), **m["bits8"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
