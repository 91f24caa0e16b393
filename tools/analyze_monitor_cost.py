"""Cost of the monitored analysis mode (AMTGPU_ANALYZE_LINEAR_MONITORED) against the guarded linear mode it extends.

The bench's headline clip (10 000 frames of 1440x1080i, 8 bit, logo 256x128 at (1120, 64), maskratio 0.35) is analysed on the device
with amtgpu_analyze_batch, timed with events on the launch stream: mode 1 and mode 3 alternated, `--reps` each after warm-up; then the
exact mode's run(), one batch that trips the monitor (re-armed with a tolerance of half the sentinel error it observed) and one batch
after the host has seen the downgrade.  Also checks that a passing batch hands out mode 1's records off the sentinels and the exact
ones on them, and that the tripped batch hands out the exact mode's records.  Writes <out>/monitor_cost.json; exits 1 when a check fails.

    python tools/analyze_monitor_cost.py [--reps 40] [--warmup 5] [--out DIR]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

W, H, PITCH_Y = 1440, 1080, 1472
LW, LH, IMGX, IMGY = 256, 128, 1120, 64
MASKRATIO = 0.35
N = 10000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=".")
    a = ap.parse_args()

    import numpy as np
    import torch

    import amt_synth as S
    from amatsukaze_amd import AMTAnalyzeLogo, Context, Logo

    dev = torch.device("cuda:0")
    ctx = Context(0)                    # launches on torch's current stream: the events below bracket exactly the library's work
    data, alpha, alphaUV = S.make_logo(LW, LH)
    Y = S.make_clip_torch(N, W, H, 0x5EED0004, alpha, alphaUV, IMGX, IMGY, dev, period=900, fade=12, pitchY=PITCH_Y, chroma=False)["Y"]
    torch.cuda.synchronize()
    logo = Logo.from_planes(ctx, data, LW, LH, W, H, IMGX, IMGY)
    lin = AMTAnalyzeLogo(ctx, logo, MASKRATIO, mode="linear")
    mon = AMTAnalyzeLogo(ctx, logo, MASKRATIO, mode="monitored")
    exact = AMTAnalyzeLogo(ctx, logo, MASKRATIO)
    out = torch.empty((N, 33), dtype=torch.float32, device=dev)

    def timed(an):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        an.analyze_device(Y, 8, out)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        timed(lin)
        timed(mon)
    t1, t3 = [], []
    for _ in range(a.reps):
        t1.append(timed(lin))
        t3.append(timed(mon))
    st = mon.monitor_stats()
    assert not st["downgraded"], st

    # records: the monitored batch = mode 1's off the sentinels, the exact mode's on them
    timed(lin)
    rec1 = out.cpu().numpy().copy()
    timed(exact)
    rec_exact = out.cpu().numpy().copy()
    mon.set_mode("monitored")
    timed(mon)
    rec3 = out.cpu().numpy().copy()
    sent = [j * (N - 1) // 15 for j in range(16)]
    other = np.setdiff1d(np.arange(N), sent)
    passing_ok = rec3[other].tobytes() == rec1[other].tobytes() and rec3[sent].tobytes() == rec_exact[sent].tobytes()
    smax = float(mon.monitor_stats()["max_abs"])

    # one tripped batch (a fresh arming with a tolerance below what the sentinels show), and the exact mode
    t_exact = [timed(exact) for _ in range(5)]
    tripped_ms, tripped_ok = None, None
    if smax > 0:
        mon.set_monitor(smax / 2, 16)
        mon.set_mode("monitored")
        tripped_ms = timed(mon)
        tripped_ok = out.cpu().numpy().tobytes() == rec_exact.tobytes() and mon.monitor_stats()["downgraded"]
        after_ms = timed(mon)          # the host has seen the flag: run() directly
    else:
        after_ms = None

    m1, m3 = statistics.median(t1), statistics.median(t3)
    res = {
        "clip": {"frames": N, "size": f"{W}x{H}i", "bits": 8, "logo": f"{LW}x{LH}@({IMGX},{IMGY})", "maskratio": MASKRATIO},
        "reps": a.reps, "warmup": a.warmup,
        "mode1_ms_median": round(m1, 4), "mode3_ms_median": round(m3, 4),
        "mode3_minus_mode1_ms_median": round(m3 - m1, 4),
        "mode3_minus_mode1_ms_median_of_pairs": round(statistics.median([b - x for x, b in zip(t1, t3)]), 4),
        "mode1_ms_min": round(min(t1), 4), "mode3_ms_min": round(min(t3), 4),
        "target_ms": 0.05,
        "exact_run_ms_median": round(statistics.median(t_exact), 4),
        "tripped_batch_ms": None if tripped_ms is None else round(tripped_ms, 4),
        "downgraded_batch_ms": None if after_ms is None else round(after_ms, 4),
        "sentinel_max_abs": smax,
        "passing_batch_records_ok": passing_ok,
        "tripped_batch_equals_exact": tripped_ok,
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "monitor_cost.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not passing_ok or tripped_ok is False:
        sys.exit(1)


if __name__ == "__main__":
    main()
