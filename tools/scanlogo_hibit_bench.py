#!/usr/bin/env python3
"""The streamed ScanLogo session at 8 and 10 bits on the bench shape (profiles/scanlogo_hibit.json).

1440x1080 frames, rectangle 256x128 at (1120, 64), 4 096 resident frames from tools/amt_synth.make_clip_torch (one frame in four
flat-bordered, no quota: every valid frame is kept), fed to a session in batches of 1 024, then finish.  Host clock around feed + finish +
a synchronise of the context, after a warm-up.

  --time OUT [--reps N] [--parent LIB]   per depth: median and min-max seconds of N repetitions of the library under amatsukaze_amd/.
                                         With --parent (a libamt_gpu.so of the parent commit, 8-bit entry points only) the 8-bit
                                         repetitions alternate parent, change, parent, ... in this one process and the condition
                                         "8-bit must not pay" is evaluated: change's median <= parent's median + parent's (max - min).
  --once BITS OUT                        one warm-up and one timed session at that depth; writes {kept, bytes the keep kernel moved}:
                                         the run to put under `rocprofv3 --kernel-trace --stats`
  --collect OUT TIME8_10 ONCE8 CSV8 ONCE10 CSV10   merges a --time result with the two profiled runs' scan_keep_kernel rows into OUT

Both libraries are loaded with plain ctypes (the parent lacks the symbols the package's binding insists on)."""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, H, LW, LH, X, Y0, SEED = 1440, 1080, 256, 128, 1120, 64, 0x5EED00C3
FRAMES, BATCH, FLAT, THY, NOMAX = 4096, 1024, 4, 12, 1 << 30
CHANGE = os.path.join(ROOT, "amatsukaze_amd", "libamt_gpu.so")


def load(path):
    lib = C.CDLL(path)
    p, i, i64, s = C.c_void_p, C.c_int, C.c_int64, C.c_char_p
    sigs = {
        "amtgpu_context_create": (p, [i]),
        "amtgpu_context_destroy": (None, [p]),
        "amtgpu_context_synchronize": (i, [p]),
        "amtgpu_last_error": (s, [p]),
        "amtgpu_scanlogo_stream_create": (p, [p] + [i] * 8),
        "amtgpu_scanlogo_stream_create_bits": (p, [p] + [i] * 9),
        "amtgpu_scanlogo_stream_destroy": (None, [p]),
        "amtgpu_scanlogo_stream_feed": (i, [p, p, p, p, i64, i64, i, i, i, p, p]),
        "amtgpu_scanlogo_stream_finish": (i, [p, i, s, p]),
    }
    for name, (res, args) in sigs.items():
        f = getattr(lib, name, None)
        if f is not None:
            f.restype, f.argtypes = res, args
    return lib


def make_clip(bits):
    import torch

    import amt_synth as S
    _, alpha, alphaUV = S.make_logo(LW, LH)
    c = S.make_clip_torch(FRAMES, W, H, SEED, alpha, alphaUV, X, Y0, torch.device("cuda:0"), bits=bits, period=900, fade=12, flat_every=FLAT)
    torch.cuda.synchronize()
    return c


def session(lib, ctx, clip, bits, out, new_entry):
    """feed + finish + synchronise; returns (seconds, kept, sha256 of the .lgd)"""
    es = 1 if bits <= 8 else 2
    Y, U, V = clip["Y"], clip["U"], clip["V"]
    if os.path.exists(out):
        os.remove(out)
    t0 = time.perf_counter()
    if new_entry:
        h = lib.amtgpu_scanlogo_stream_create_bits(ctx, W, H, bits, X, Y0, LW, LH, THY, NOMAX)
    else:
        h = lib.amtgpu_scanlogo_stream_create(ctx, W, H, X, Y0, LW, LH, THY, NOMAX)
    if not h:
        raise RuntimeError(lib.amtgpu_last_error(ctx).decode(errors="replace"))
    nk = C.c_int()
    for f0 in range(0, FRAMES, BATCH):
        y, u, v = Y[f0:f0 + BATCH], U[f0:f0 + BATCH], V[f0:f0 + BATCH]
        ok = lib.amtgpu_scanlogo_stream_feed(h, y.data_ptr(), u.data_ptr(), v.data_ptr(), Y.stride(0) * es, U.stride(0) * es, Y.stride(1),
                                             U.stride(1), int(y.shape[0]), C.byref(nk), None)
        if not ok:
            raise RuntimeError(lib.amtgpu_last_error(ctx).decode(errors="replace"))
    ok = lib.amtgpu_scanlogo_stream_finish(h, 1041, out.encode(), None)
    lib.amtgpu_context_synchronize(ctx)
    dt = time.perf_counter() - t0
    if not ok:
        raise RuntimeError(lib.amtgpu_last_error(ctx).decode(errors="replace"))
    lib.amtgpu_scanlogo_stream_destroy(h)
    return dt, nk.value, hashlib.sha256(open(out, "rb").read()).hexdigest()


def spread(xs):
    return {"median_s": round(statistics.median(xs), 5), "min_s": round(min(xs), 5), "max_s": round(max(xs), 5), "seconds": [round(x, 5) for x in xs]}


def run_time(out, reps, parent):
    import torch
    res = {"shape": f"{W}x{H}", "rect": [X, Y0, LW, LH], "frames": FRAMES, "batch": BATCH, "flat_every": FLAT, "reps": reps,
           "clock": "host perf_counter around create + feeds + finish + amtgpu_context_synchronize"}
    change = load(CHANGE)
    cctx = change.amtgpu_context_create(0)
    tmp = out + ".lgd"
    for bits in (8, 10):
        clip = make_clip(bits)
        libs = [("change", change, cctx, True)]
        if bits == 8 and parent:
            plib = load(parent)
            libs.insert(0, ("parent", plib, plib.amtgpu_context_create(0), False))
        times = {tag: [] for tag, *_ in libs}
        sha, kept = {}, {}
        for tag, lib, ctx, new_entry in libs:                   # warm-up
            session(lib, ctx, clip, bits, tmp, new_entry)
        for _ in range(reps):
            for tag, lib, ctx, new_entry in libs:               # alternated
                dt, k, h = session(lib, ctx, clip, bits, tmp, new_entry)
                times[tag].append(dt)
                sha[tag], kept[tag] = h, k
        r = {"kept": kept["change"], "feed_plus_finish": spread(times["change"]), "lgd_sha256": sha["change"]}
        if "parent" in times:
            p, c = spread(times["parent"]), r["feed_plus_finish"]
            r["parent_feed_plus_finish"] = p
            r["lgd_equals_parent"] = sha["parent"] == sha["change"]
            allowed = p["median_s"] + (p["max_s"] - p["min_s"])
            r["eight_bit_must_not_pay"] = {"rule": "change median <= parent median + (parent max - parent min)", "allowed_s": round(allowed, 5),
                                           "holds": c["median_s"] <= allowed}
        res[f"bits{bits}"] = r
        del clip
        torch.cuda.empty_cache()
    if os.path.exists(tmp):
        os.remove(tmp)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res), flush=True)
    return 0


def run_once(bits, out):
    lib = load(CHANGE)
    ctx = lib.amtgpu_context_create(0)
    clip = make_clip(bits)
    tmp = out + ".lgd"
    session(lib, ctx, clip, bits, tmp, True)
    dt, kept, _ = session(lib, ctx, clip, bits, tmp, True)
    es = 1 if bits <= 8 else 2
    rect_bytes = (LW * LH + 2 * (LW // 2) * (LH // 2)) * es
    os.remove(tmp)
    # two sessions (warm-up and timed), FRAMES / BATCH launches each; a kept rectangle is read once and written once
    res = {"bits": bits, "kept_per_session": kept, "sessions": 2, "launches": 2 * (FRAMES // BATCH), "bytes_moved": 2 * 2 * kept * rect_bytes,
           "seconds_under_profiler": round(dt, 5)}
    json.dump(res, open(out, "w"))
    print(json.dumps(res), flush=True)
    return 0


def keep_row(path):
    for row in csv.DictReader(open(path)):
        if "scan_keep_kernel" in row.get("Name", ""):
            return {"calls": int(row["Calls"]), "total_ns": int(row["TotalDurationNs"]), "mean_ns": float(row["AverageNs"])}
    raise RuntimeError(f"no scan_keep_kernel row in {path}")


def run_collect(out, timed, *pairs):
    res = json.load(open(timed))
    for once, stats in zip(pairs[0::2], pairs[1::2]):
        o, k = json.load(open(once)), keep_row(stats)
        k["bytes_moved"] = o["bytes_moved"]
        k["GB_per_s"] = round(o["bytes_moved"] / k["total_ns"], 2)
        k["source"] = "rocprofv3 --kernel-trace --stats, a run of its own (two sessions of four feeds)"
        res[f"bits{o['bits']}"]["scan_keep_kernel"] = k
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent")
    ap.add_argument("--once", nargs=2, metavar=("BITS", "OUT"))
    ap.add_argument("--collect", nargs="+")
    a = ap.parse_args()
    if a.time:
        return run_time(a.time, max(5, a.reps), a.parent)
    if a.once:
        return run_once(int(a.once[0]), a.once[1])
    if a.collect:
        return run_collect(*a.collect)
    ap.error("nothing to do")


if __name__ == "__main__":
    sys.exit(main())
