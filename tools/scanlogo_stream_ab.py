#!/usr/bin/env python3
"""A/B of amtgpu_scanlogo_file between two builds of the library (profiles/scanlogo_stream.json).

  --make-clip RAW [--frames N]   writes the raw 'AMTR' clip: N frames of 352x240 8-bit from tools/amt_synth.make_clip_torch, EVERY frame
                                 flat-bordered (flat_every=1), so that numMaxFrames = N keeps them all -- the case in which the reader
                                 moves the most rectangles
  --time LIB RAW OUT             loads LIB (a libamt_gpu.so of either build) with plain ctypes, runs amtgpu_scanlogo_file over RAW with
                                 numMaxFrames = the clip's length and a host clock around the call (it ends in a synchronise), prints one
                                 JSON line {lib, seconds, ok, error, lgd_sha256}

One measurement per process: the caller alternates the two builds and gives every run its own time limit."""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, H, LW, LH, X, Y0, SEED, THY = 352, 240, 96, 48, 224, 18, 0x5EED00B7, 12


def make_clip(path: str, frames: int, piece: int = 2000) -> None:
    import numpy as np
    import torch

    import amt_synth as S
    _, alpha, alphaUV = S.make_logo(LW, LH)
    dev = torch.device("cuda:0")
    ysz, csz = W * H, (W // 2) * (H // 2)
    with open(path, "wb") as f:
        f.write(np.array([0x52544D41, W, H, frames], np.int32).tobytes())
        for f0 in range(0, frames, piece):
            n = min(piece, frames - f0)
            c = S.make_clip_torch(n, W, H, SEED, alpha, alphaUV, X, Y0, dev, period=900, fade=12, start=f0, flat_every=1)
            out = np.empty((n, ysz + 2 * csz), np.uint8)            # file order: Y, U, V of one frame back to back
            out[:, :ysz] = c["Y"].cpu().numpy().reshape(n, ysz)
            out[:, ysz:ysz + csz] = c["U"].cpu().numpy().reshape(n, csz)
            out[:, ysz + csz:] = c["V"].cpu().numpy().reshape(n, csz)
            f.write(out.tobytes())
    print(json.dumps({"clip": path, "frames": frames, "bytes": os.path.getsize(path)}), flush=True)


def time_one(libpath: str, raw: str, out: str) -> int:
    lib = C.CDLL(libpath)
    lib.amtgpu_context_create.restype = C.c_void_p
    lib.amtgpu_context_create.argtypes = [C.c_int]
    lib.amtgpu_context_destroy.argtypes = [C.c_void_p]
    lib.amtgpu_last_error.restype = C.c_char_p
    lib.amtgpu_last_error.argtypes = [C.c_void_p]
    lib.amtgpu_scanlogo_file.restype = C.c_int
    lib.amtgpu_scanlogo_file.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p] + [C.c_int] * 6 + [C.c_void_p]
    with open(raw, "rb") as f:
        frames = int.from_bytes(f.read(16)[12:16], "little")
    ctx = lib.amtgpu_context_create(0)
    if not ctx:
        print(json.dumps({"lib": libpath, "ok": False, "error": "no context"}), flush=True)
        return 1
    if os.path.exists(out):
        os.remove(out)
    t0 = time.perf_counter()
    ok = lib.amtgpu_scanlogo_file(ctx, raw.encode(), 1041, b"", out.encode(), X, Y0, LW, LH, THY, frames, None)
    dt = time.perf_counter() - t0
    err = "" if ok else lib.amtgpu_last_error(ctx).decode(errors="replace")
    sha = hashlib.sha256(open(out, "rb").read()).hexdigest() if ok and os.path.exists(out) else None
    lib.amtgpu_context_destroy(ctx)
    print(json.dumps({"lib": libpath, "frames": frames, "seconds": round(dt, 4), "ok": bool(ok), "error": err, "lgd_sha256": sha}), flush=True)
    return 0 if ok else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--make-clip")
    ap.add_argument("--frames", type=int, default=20000)
    ap.add_argument("--time", nargs=3, metavar=("LIB", "RAW", "OUT"))
    a = ap.parse_args()
    if a.make_clip:
        make_clip(a.make_clip, a.frames)
        return 0
    if a.time:
        return time_one(*a.time)
    ap.error("nothing to do")
    return 2


if __name__ == "__main__":
    sys.exit(main())
