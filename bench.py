#!/usr/bin/env python3
"""bench.py -- frames/sec of the logo + CM + KFM analysis pass on synthetic 1440x1080i YUV420 (BASELINE.json).

One "step" = one pass of the hot path over one HBM-resident batch of frames (config.workload, BASELINE configs[1]):
    AMTAnalyzeLogo (33 evaluations per frame, LogoScan.hpp:1119-1161)
 -> LogoFrame scan (2 candidate logos + 1 erase logo, :1543-1568) and the whole-frame field-difference / combing
    metrics (self-specified CM / KFM pass) on the source frames, while the host turns the analysis records into fades
 -> CalcFade on the device (:1317-1341, amtgpu_erase_calc_fades_device)  -> AMTEraseLogo in place (:1248-1261, :1374-1397)
Inputs are already in HBM when the timed region starts.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--scaling weak|strong] [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times the K steps and prints the line: `value` (frames/sec) and `ms_per_step` are those of
the timed steps.  --dump-outputs DIR writes what the last timed step computed to DIR/<name>.npy (float32, or float64 for
integer sums), inputs identical from run to run, so that two builds can be compared output for output.  Everything else
described below -- per-kernel timing and `roofline`, the CPU oracle check (`verified`), `exact_mode`, `in_place_erase_step`,
the other analysis mode, `strong_scan`, `configs`, `e2e10`, `boundary`, `ingest`, `cpu_baseline` -- runs with --full only.

--gpus N > 1 without a torch.distributed environment re-executes itself under torch.distributed.run (one rank per GPU,
RCCL); the driver's own `python -m torch.distributed.run ... bench.py --gpus N` is used as it comes.
  * weak (default): every rank owns its own 10 000-frame batch; the scan's {corr0,corr1} records are all-gathered
    (the one real exchange of the all-frames scan; rank 0 decides).
  * strong: BASELINE configs[3] -- the 107 892-frame (60 min) Y-only LogoFrame scan sharded by contiguous frame range,
    records all-gathered, rank 0 runs selectLogo / writeResult; total work fixed as N grows.  The same measurement is
    also attached to the default line as `strong_scan`.

After the timed steps the batch is regenerated and ONE more step at the same launch geometry is checked against the
CPU oracle on sampled frame blocks (`verified`); a mismatch exits non-zero.  Prints ONE JSON line (rank 0).
`roofline` describes the dominant kernel, timed with HIP events on the launch stream inside the timed steps;
`cpu_baseline` is the CPU oracle (restatement of the reference, pinned against the real reference sources) on a bounded
sample of the same workload: single thread (`value`) and all host cores (`all_cores`).
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np

W, H = 1440, 1080
PITCH_Y, PITCH_UV = 1472, 768          # AviSynth planes are 64-byte aligned (include/avs/config.h:45)
LW, LH, IMGX, IMGY = 256, 128, 1120, 64
MASKRATIO = 0.35                       # CMAnalyze.hpp:291 / AMTAnalyzeLogo default
FLOPS_PER_MASK_PIXEL = 101             # mean 20+4 adds + 1 div, corr 25 sub + 25 mul + 20+4 adds, score 2 mul
FLOPS_PER_RECT_PIXEL = 6               # EvaluateLogo's unblend per rectangle pixel per evaluation (LogoScan.hpp:244-249)
HBM_PEAK_GBS = 8000.0                  # MI355X_MICROARCH.md
FP32_PEAK_TFLOPS = 157.3               # fp32 vector peak (FMA counted as 2)
STRONG_FRAMES = 107892                 # BASELINE configs[3]: 60 min at 29.97 fps
SCANLOGO_MAX_FRAMES = 20000            # ScanLogo's numMaxFrames (LogoScan.hpp:885)
SCANLOGO_FLAT_EVERY = 4                # one frame in four passes AddFrame's border test: 26 9xx of 107 892 > numMaxFrames, so the stream-order
                                       # quota closes the stream early (round 5: one in eight, 13 486 accepted -- the quota was never reached)
PMC_TRAFFIC = os.path.join("profiles", "r06_pmc_traffic.json")
EVAL = "logo_eval_fused_kernel"


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=320, help="timed steps (default: a >= 5 s timed region)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    ap.add_argument("--frames", type=int, default=10000, help="frames per GPU batch (BASELINE configs[1]: 10k)")
    ap.add_argument("--strong-frames", type=int, default=STRONG_FRAMES, help="frames of the sharded all-frames scan (configs[3])")
    ap.add_argument("--strong-steps", type=int, default=20)
    ap.add_argument("--scanlogo-max-frames", type=int, default=SCANLOGO_MAX_FRAMES,
                    help="numMaxFrames of the ScanLogo runs (LogoScan.hpp:885: the first so many valid frames in stream order); small values let a "
                         "short dry run reach the quota")
    ap.add_argument("--no-strong", action="store_true", help="skip the attached strong-scaling scan measurement")
    ap.add_argument("--cpu-frames", type=int, default=300, help="distinct frames of the CPU baseline sample (configs[0]: 300; 0 = skip)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="repeat the CPU sample until this much CPU work is timed")
    ap.add_argument("--no-ingest", action="store_true", help="skip the PCIe-inclusive (streamed) measurement")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--no-erase", action="store_true")
    ap.add_argument("--erase-in-place", action="store_true",
                    help="rounds 1-5: AMTEraseLogo rewrites the resident frames in place and the step puts the rectangles back afterwards (bench "
                         "housekeeping inside the timed region, ~0.4 ms).  Default: Delogo reads the resident frames and writes the rectangle into a "
                         "second resident batch that holds a copy of them -- the writable copy AMTEraseLogo::GetFrameT takes (env->MakeWritable, "
                         "LogoScan.hpp:1346-1347; amtgpu_erase_batch_dfades_to): the same reads and writes, nothing to put back")
    ap.add_argument("--no-alt-mode", action="store_true", help="do not time the other analysis mode after the timed region (profiling runs)")
    ap.add_argument("--no-configs", action="store_true", help="skip the attached measurements of BASELINE configs[2], the 10-bit format and ScanLogo")
    ap.add_argument("--exact-steps", type=int, default=40, help="timed steps of the same pass with the exact (bit-identical) analysis, reported as exact_mode")
    ap.add_argument("--workload", choices=("headline", "e2e10"), default="headline",
                    help="e2e10: BASELINE configs[4] (tools/bench_e2e.py) as the line's own workload, frames sharded over --gpus ranks (strong scaling)")
    ap.add_argument("--e2e-frames", type=int, default=0, help="TOTAL frames of the e2e10 stream, sharded over the ranks (strong scaling).  Default 0: 53 946 "
                                                              "frames per rank = one GPU's share of the 4-hour stream, so N = 8 runs the whole 431 568-frame "
                                                              "stream of configs[4] (weak scaling)")
    ap.add_argument("--e2e-chunk", type=int, default=4096, help="frames generated and processed per chunk of the e2e10 stream")
    ap.add_argument("--e2e-verify-seconds", type=float, default=150.0,
                    help="wall-time budget per rank for holding every frame of its e2e10 share against the CPU oracle; chunks beyond it are left to the "
                         "probe blocks and the line says so (verified_whole_stream).  One share of 53 946 frames is 42 s of a 256-core host; the ranks "
                         "of a node share its cores, so N shares take N x 42 s: whole at N <= 2 (and N = 3), ~90 % at N = 4, ~45 % at N = 8 under the default -- the "
                         "oracle's speed, not the GPUs', bounds it, and the default run has to stay within minutes")
    ap.add_argument("--metrics-cus", type=int, default=0,
                    help="N > 0: N compute units are given to the frame metrics, which then run BESIDE the analysis + scan on the other units (two contexts "
                         "on CU-range streams, amtgpu_stream_create_cu_range).  Measured (profiles/r04_notes.md): no gain on MI355X -- the logo kernels lose "
                         "what the metrics gain -- so the default 0 keeps every kernel on the whole device, one pass after the other")
    ap.add_argument("--fades", choices=("device", "host"), default="device",
                    help="where CalcFade runs inside the step: device = amtgpu_erase_calc_fades_device, the whole step stream-ordered (default); "
                         "host = round 3's step (records to the host, host CalcFade while the scan runs, fades back up)")
    ap.add_argument("--no-e2e", action="store_true", help="do not attach the e2e10 measurement to the default line")
    ap.add_argument("--analysis-mode", choices=("linear", "exact"), default="linear",
                    help="AMTAnalyzeLogo evaluation: linear = all fades from one window evaluation of s and bg, decisions guarded by exact "
                         "re-evaluation (identical fades / erased frames, scores within 1e-4); exact = the reference's fp32 order for every fade")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: per-kernel timing and roofline, verification against the CPU oracle, the exact-mode and in-place "
                         "erase steps, the other analysis mode, the strong scan, the other configurations, e2e10, boundary, ingest, CPU baseline "
                         "(each still subject to its own --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (rank 0; at most 64 MB, a fixed seeded "
                         "sample of frames where the whole output is larger)")
    return ap.parse_args()


def respawn_under_torchrun(args):
    """`python bench.py --gpus N` with no rendezvous environment: start N ranks (one per GPU) and relay their exit code"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, env=env))


def make_logos():
    import amt_synth as S
    main, alpha, alphaUV = S.make_logo(LW, LH)
    cand2, _, _ = S.make_logo(LW, LH, seed=0x10600002, strength=0.5)
    cand3, _, _ = S.make_logo(LW, LH, seed=0x10600003, strength=0.8)
    return (main, cand2, cand3), alpha, alphaUV


def _ptr_np(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class OracleLogos:
    """the checker's evaluation logos: deint of every candidate + top/bottom field logos of the erase logo"""

    def __init__(self, logos_np, W=W, H=H, imgx=IMGX, imgy=IMGY, bits=8):
        from amtlib import Oracle
        self.orc = orc = Oracle()
        self.W, self.H, self.bits = W, H, bits
        self.hs = [orc.make_logo(d, LW, LH, W, H, imgx, imgy) for d in logos_np]
        self.deints = []
        for h in self.hs:
            d = orc.lib.orc_logo_deint(h)
            orc.lib.orc_logo_create_mask(d, MASKRATIO, 1)
            self.deints.append(d)
        self.top = orc.lib.orc_logo_field(self.hs[0], 0); orc.lib.orc_logo_create_mask(self.top, MASKRATIO, 1)
        self.bot = orc.lib.orc_logo_field(self.hs[0], 1); orc.lib.orc_logo_create_mask(self.bot, MASKRATIO, 1)
        self.deint_arr = (C.c_void_p * len(self.deints))(*self.deints)

    def scan(self, Y, n):
        ev = np.zeros(n * len(self.deints) * 2, np.float32)
        self.orc.lib.orc_logoframe_scan(self.deint_arr, len(self.deints), _ptr_np(Y), Y.strides[0], Y.shape[2], self.bits, self.W, self.H, n, _ptr_np(ev))
        return ev

    def analyze(self, Y, n):
        an = np.zeros(n * 33, np.float32)
        self.orc.lib.orc_analyze_frames(self.deints[0], self.top, self.bot, _ptr_np(Y), Y.strides[0], Y.shape[2], self.bits, n, _ptr_np(an))
        return an

    def fade(self, an, n, i):
        ft, fb = C.c_float(), C.c_float()
        self.orc.lib.orc_calc_fade(None, 0, 16, _ptr_np(an), n, i, C.byref(ft), C.byref(fb))
        return ft.value, fb.value

    def erase(self, Y, U, V, i, ft, fb):
        self.orc.lib.orc_erase_frame(self.hs[0], _ptr_np(Y[i]), _ptr_np(U[i]), _ptr_np(V[i]), Y.shape[2], U.shape[2], self.bits, ft, fb)

    def metrics(self, Y, n, prev=None):
        fs = np.zeros((n, 8), np.uint64)
        self.orc.lib.orc_frame_metrics(_ptr_np(Y), Y.strides[0], Y.shape[2], self.bits, self.W, self.H, n, _ptr_np(prev), _ptr_np(fs))
        return fs


# --------------------------------------------------------------------------------------------------------------------
# CPU baseline (rank 0, N=1 only): the oracle on a bounded sample of the same pass
# --------------------------------------------------------------------------------------------------------------------
def cpu_baseline(nframes, logos_np, alpha, alphaUV, min_seconds):
    """Returns the `cpu_baseline` object.  Single thread: the reference's own loops are serial (LogoScan.hpp:1577).
    All cores: the same per-frame work dealt over threads (ctypes releases the GIL; the oracle keeps no shared state)."""
    import amt_synth as S
    from concurrent.futures import ThreadPoolExecutor
    ol = OracleLogos(logos_np)
    orc = ol.orc
    clip = S.make_clip_np(nframes, W, H, 0x5EED0001, alpha, alphaUV, IMGX, IMGY, period=24, fade=6, pitchY=PITCH_Y, pitchUV=PITCH_UV)
    Y0, U0, V0 = clip["Y"], clip["U"], clip["V"]
    Y, U, V = Y0.copy(), U0.copy(), V0.copy()
    detail = {"scan_s": 0.0, "analyze_s": 0.0, "fade_erase_s": 0.0, "frame_metrics_s": 0.0}
    total, frames_timed = 0.0, 0
    first = None
    while total < min_seconds:           # the whole pass over the sample, repeated
        np.copyto(Y, Y0); np.copyto(U, U0); np.copyto(V, V0)   # erase rewrites the sample in place (untimed restore)
        t0 = time.perf_counter()
        ev = ol.scan(Y, nframes)
        t1 = time.perf_counter()
        an = ol.analyze(Y, nframes)
        t2 = time.perf_counter()
        fs = ol.metrics(Y, nframes)
        t3 = time.perf_counter()
        for i in range(nframes):
            ft, fb = ol.fade(an, nframes, i)
            ol.erase(Y, U, V, i, ft, fb)
        t4 = time.perf_counter()
        total += t4 - t0
        frames_timed += nframes
        for k, dt in zip(detail, (t1 - t0, t2 - t1, t4 - t3, t3 - t2)):
            detail[k] += dt
        if first is None:
            first = (ev, an)
    single = frames_timed / total
    logo_only = frames_timed / (detail["scan_s"] + detail["analyze_s"] + detail["fade_erase_s"])

    # ---- all host cores: frames dealt round-robin to threads, two phases (fades need every frame's analysis) ----
    ncpu = os.cpu_count() or 1
    try:
        ncpu = len(os.sched_getaffinity(0))
    except Exception:
        pass
    T = max(1, min(ncpu, nframes))
    an_all = np.zeros(nframes * 33, np.float32)
    ev_all = np.zeros(nframes * len(ol.deints) * 2, np.float32)
    fs_all = np.zeros((nframes, 8), np.uint64)
    nl = len(ol.deints)

    def phase1(t):
        for i in range(t, nframes, T):
            orc.lib.orc_logoframe_scan(ol.deint_arr, nl, _ptr_np(Y0[i]), Y0.strides[0], Y0.shape[2], 8, W, H, 1,
                                       C.c_void_p(ev_all.ctypes.data + i * nl * 8))
            orc.lib.orc_analyze_frames(ol.deints[0], ol.top, ol.bot, _ptr_np(Y0[i]), Y0.strides[0], Y0.shape[2], 8, 1,
                                       C.c_void_p(an_all.ctypes.data + i * 33 * 4))
            orc.lib.orc_frame_metrics(_ptr_np(Y0[i]), Y0.strides[0], Y0.shape[2], 8, W, H, 1, _ptr_np(Y0[max(0, i - 1)]),
                                      C.c_void_p(fs_all.ctypes.data + i * 64))

    def phase2(t):
        y = np.empty_like(Y0[0]); u = np.empty_like(U0[0]); v = np.empty_like(V0[0])
        for i in range(t, nframes, T):
            ft, fb = ol.fade(an_all, nframes, i)
            np.copyto(y, Y0[i]); np.copyto(u, U0[i]); np.copyto(v, V0[i])      # MakeWritable's copy (LogoScan.hpp:1361)
            orc.lib.orc_erase_frame(ol.hs[0], _ptr_np(y), _ptr_np(u), _ptr_np(v), Y0.shape[2], U0.shape[2], 8, ft, fb)

    mt_total, mt_frames = 0.0, 0
    with ThreadPoolExecutor(T) as ex:
        while mt_total < max(2.0, min_seconds / 3):
            t0 = time.perf_counter()
            list(ex.map(phase1, range(T)))
            list(ex.map(phase2, range(T)))
            mt_total += time.perf_counter() - t0
            mt_frames += nframes
    assert an_all.tobytes() == first[1].tobytes() and ev_all.tobytes() == first[0].tobytes(), "threaded oracle differs from the serial one"

    ref_check = reference_logo_passes(orc, ol.hs, Y0, U0, V0, min(nframes, 64), first)
    return {"value": single, "unit": "frames/sec", "cores": 1, "kind": "port",
            "sample": f"{frames_timed} frames ({nframes} distinct 1440x1080 8-bit frames = BASELINE configs[0]'s clip length, pass repeated), same "
                      "pass as the GPU step (scan 3 logos + analyze + frame metrics + fade/erase), oracle/libamt_oracle.so -O2 -mavx, "
                      "single thread (the reference's loops are serial, LogoScan.hpp:1577)",
            "logo_passes_only_fps": logo_only,
            "all_cores": {"value": mt_frames / mt_total, "unit": "frames/sec", "cores": T, "host_cpus": os.cpu_count(),
                          "sample": f"{mt_frames} frames, frames dealt over {T} threads (ctypes releases the GIL), two phases "
                                    "(scan+analysis+metrics, then fade+erase on a copy of the frame)"},
            "detail_s": detail, "reference_check": ref_check}


def reference_logo_passes(orc, hs, Y, U, V, nframes, oracle_out):
    """The REAL reference (oracle/_ref/libamt_ref.so: LogoScan.hpp / ComputeKernel.cpp compiled through oracle/ref_shim) on the
    first `nframes` frames of the sample: LogoFrame scan and AMTAnalyzeLogo, timed AND byte-compared with the oracle's output
    for the same frames.  None where the library was never built (it needs /root/reference at build time)."""
    import tempfile
    from amtlib import Ref
    if not Ref.available():
        return None
    ref = Ref()
    tmp = tempfile.mkdtemp()
    paths = []
    for i, h in enumerate(hs):
        p = os.path.join(tmp, f"logo{i}.lgd").encode()
        if not orc.lib.orc_logo_save(h, p, b"bench", 1):
            return None
        paths.append(p)
    nl = len(hs)
    ev = np.zeros(nframes * nl * 2, np.float32)
    best, ratio = C.c_int(), C.c_float()
    text = C.create_string_buffer(1 << 20)
    t0 = time.perf_counter()
    ok = ref.lib.ref_logoframe((C.c_char_p * nl)(*paths), nl, MASKRATIO, _ptr_np(Y), Y.strides[0], Y.shape[2], 8, W, H, nframes, 30000, 1001,
                               _ptr_np(ev), nl, C.byref(best), C.byref(ratio), -1, os.path.join(tmp, "logof.txt").encode(), text, len(text))
    t1 = time.perf_counter()
    an = np.zeros(nframes * 33, np.float32)
    ok2 = ref.lib.ref_analyze(paths[0], MASKRATIO, _ptr_np(Y), _ptr_np(U), _ptr_np(V), Y.strides[0], U.strides[0], Y.shape[2], U.shape[2], 8,
                              W, H, nframes, _ptr_np(an))
    t2 = time.perf_counter()
    if ok != 1 or ok2 != 1:
        raise SystemExit("reference_check: the reference build failed to run: " + str(ref.lib.ref_last_error()))
    same_scan = ev.tobytes() == oracle_out[0][:nframes * nl * 2].tobytes()
    same_an = an.tobytes() == oracle_out[1][:nframes * 33].tobytes()
    if not (same_scan and same_an):
        raise SystemExit(f"reference_check FAILED at 1440x1080: oracle != real reference (scan equal: {same_scan}, analysis equal: {same_an})")
    return {"kind": "reference", "frames": nframes, "scan_s": t1 - t0, "analyze_s": t2 - t1, "oracle_equals_reference": True,
            "note": "real LogoScan.hpp/ComputeKernel.cpp through oracle/ref_shim; includes each filter instance's one-off CreateLogoMask; "
                    "outputs byte-compared with the oracle's for the same 1440x1080 frames"}


# --------------------------------------------------------------------------------------------------------------------
# verification of the bench's own outputs (outside the timed region)
# --------------------------------------------------------------------------------------------------------------------
def tolerance_accounting(lin, exact, fades_lin, eraser, analyzer, N):
    """Every score of the linear-guarded step against the exact kernel's (= the reference's bytes) on the same frames, and every
    fade pair.  The scores are normalised correlations (CorrelationScore / blackScore: 1.0 = the logo on black, LogoScan.hpp:254)
    that cross zero at the best fade, so 'relative' needs a floor: rel = |d| / max(|ref|, floor), reported for several floors.
    The gate (north star: "within 1e-4 relative"): rel <= 1e-4 with floor 1e-3 -- which implies |d| <= 1e-4 -- and fades
    identical on every frame."""
    d = np.abs(lin.astype(np.float64) - exact.astype(np.float64))
    a = np.abs(exact.astype(np.float64))
    out = {"analysis_scores_compared": int(d.size), "analysis_max_abs": float(d.max()),
           "analysis_max_rel": {f"floor_{fl:g}": float((d / np.maximum(a, fl)).max()) for fl in (1.0, 0.05, 0.01, 0.001)},
           # relative error with NO floor: unbounded by construction where the score crosses zero (the best fade); printed so that nobody has to guess
           "analysis_max_rel_no_floor": float((d[a > 0] / a[a > 0]).max()) if (a > 0).any() else 0.0,
           "guarantee": "fades (hence erased pixels) identical to the exact mode's: rigorous, guarded by exact re-evaluation; scores within "
                        "error_bound_rigorous: rigorous but loose; scores within 1e-4: an observation, checked here over the whole batch",
           "analysis_rel_gate": "rel = |lin - exact| / max(|exact|, 1e-3) <= 1e-4 over every score of the batch (scores are normalised to 1 = logo "
                                "on black and cross zero at the best fade, hence the floor)",
           "analysis_score_range": [float(exact.min()), float(exact.max())],
           "error_bound_rigorous": [float(analyzer.error_bound(k, 8)) for k in range(3)],
           "error_bound_note": "EvalEngine::linear_error_bound: worst case of every rounding conspiring, what the decision guard uses "
                               "(2x); the observed error is what this line reports"}
    fades_ex = eraser.calc_fades(exact, N)
    out["fades_compared"] = int(N)
    out["fades_equal_all"] = bool(np.ascontiguousarray(fades_ex).tobytes() == np.ascontiguousarray(fades_lin).tobytes())
    out["tolerance_ok"] = bool(out["analysis_max_abs"] <= 1e-4 and out["analysis_max_rel"]["floor_0.001"] <= 1e-4 and out["fades_equal_all"])
    return out



# --------------------------------------------------------------------------------------------------------------------
# the printed line: ONE compact JSON object (< 6 KB) as the LAST line of stdout; everything else goes to bench_detail.json
# --------------------------------------------------------------------------------------------------------------------
LINE_LIMIT = 6144
DETAIL_NAME = "bench_detail.json"


def _r(x, sig=6):
    """floats to 6 significant digits (a line that carries 17-digit floats is mostly digits)"""
    if isinstance(x, bool) or x is None:
        return x
    if isinstance(x, float):
        return float(f"{x:.{sig}g}") if x == x and abs(x) != float("inf") else None
    if isinstance(x, dict):
        return {k: _r(v, sig) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r(v, sig) for v in x]
    return x


def _pick(d, *keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


def _short(s, n=160):
    return s if not isinstance(s, str) or len(s) <= n else s[:n - 3] + "..."


def compact_line(full):
    """The driver-facing line: the contract's scalar keys, `roofline`, `roofline_second`, `cpu_baseline`, `exact_mode`, `verified` and one
    scalar per attached measurement.  Prose (`what` / `note`), per-kernel tables, sweeps and histograms stay in bench_detail.json."""
    g = lambda d, *path: (g(d.get(path[0]), *path[1:]) if len(path) > 1 else d.get(path[0])) if isinstance(d, dict) else None
    line = {k: full.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                     "vs_baseline", "dtype", "data")}
    cfg = full.get("config") or {}
    line["config"] = {k: _short(v) for k, v in cfg.items() if v is not None and not isinstance(v, dict)}
    for k in ("timed_region_s", "collectives"):
        if full.get(k) is not None:
            line[k] = full[k]

    def roof(r):
        if not r:
            return None
        o = _pick(r, "kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "flops_per_launch",
                  "algorithmic_bytes_per_launch", "cus")
        o.setdefault("traffic", None)
        if r.get("traffic_source"):
            o["traffic_source"] = r["traffic_source"].split(" ")[0]
        return o
    if "roofline" in full:
        line["roofline"] = roof(full["roofline"])
    if full.get("roofline_second"):
        line["roofline_second"] = roof(full["roofline_second"])
    cpu = full.get("cpu_baseline")
    if "cpu_baseline" in full:
        line["cpu_baseline"] = None
    if cpu:
        c = _pick(cpu, "value", "unit", "cores", "kind", "logo_passes_only_fps")
        c["sample"] = _short(cpu.get("sample_short") or cpu.get("sample"), 110)
        if cpu.get("all_cores"):
            c["all_cores"] = _pick(cpu["all_cores"], "value", "cores")
        if cpu.get("reference_check"):
            c["reference_check"] = _pick(cpu["reference_check"], "oracle_equals_reference", "frames")
        line["cpu_baseline"] = c
        line.update(_pick(full, "gpu_over_cpu", "gpu_over_cpu_all_cores"))
    if full.get("exact_mode"):
        line["exact_mode"] = _pick(full["exact_mode"], "value", "ms_per_step", "steps")
    if full.get("in_place_erase_step"):
        line["in_place_erase_step"] = _pick(full["in_place_erase_step"], "value", "ms_per_step", "steps")
    v = full.get("verified")
    if v:
        o = _pick(v, "ok", "frames", "scan", "analysis", "fades", "erase", "metrics", "oracle", "analysis_max_abs_err", "analysis_max_abs",
                  "fades_equal_all", "guard_refined_frames", "tolerance_ok", "seconds")
        rel = g(v, "analysis_max_rel", "floor_0.001")
        if rel is not None:
            o["analysis_max_rel_floor_1e-3"] = rel
        line["verified"] = o
    ks = full.get("kernels")
    if ks:      # name -> [avg launch ms, fraction of its roofline or null]: the table itself is in the detail file
        line["kernels_ms_frac"] = {n: [e.get("avg_ms"), e.get("frac_fp32_peak", e.get("frac"))] for n, e in ks.items()}
    e2e = full.get("e2e10")
    if e2e:
        line["e2e10"] = (_pick(e2e, "error") or
                         {**_pick(e2e, "value", "frames_total", "n_gpus", "scaling", "timed_s"), "verified_ok": g(e2e, "verified", "ok"),
                          "verified_frames": g(e2e, "verified", "frames_compared_with_cpu_oracle"), "verified_whole_stream": g(e2e, "verified", "whole_stream"),
                          "decisions_sha256": (e2e.get("decisions_sha256") or "")[:16]})
    cf = full.get("configs")
    if cf:
        line["configs"] = {n: (_pick(c, "error") or {**_pick(c, "value", "frames"), **({"verified_frames": g(c, "verified", "frames")}
                                                                                         if g(c, "verified", "frames") else {}),
                                                     **({"quota_hit": g(c, "verified", "quota_hit")} if g(c, "verified", "quota_hit") is not None else {})})
                           for n, c in cf.items() if isinstance(c, dict)}
    ss = full.get("strong_scan")
    if ss:
        line["strong_scan"] = (_pick(ss, "error") or
                               {**_pick(ss, "value", "frames_total", "n_gpus", "ms_per_step"), "records_sha256": (ss.get("records_sha256") or "")[:16],
                                "verified_frames": g(ss, "verified", "frames"), "verified_ok": g(ss, "verified", "equals_cpu_oracle"),
                                "scanlogo_value": g(ss, "scanlogo", "value"), "lgd_sha256": (g(ss, "scanlogo", "lgd_sha256") or "")[:16],
                                "lgd_verified_frames": g(ss, "scanlogo", "verified", "frames"), "lgd_equals_cpu_oracle": g(ss, "scanlogo", "verified", "lgd_equals_cpu_oracle"),
                                "scanlogo_quota_hit": g(ss, "scanlogo", "verified", "quota_hit")})
    ing = full.get("ingest")
    if ing:
        line["ingest"] = _pick(ing, "error") or {"y_plane": _pick(ing.get("y_plane") or {}, "pipelined_fps", "ingest_GBs"),
                                                 "logo_rows": _pick(ing.get("logo_rectangle_rows") or {}, "pipelined_fps", "ingest_GBs")}
    bd = full.get("boundary")
    if bd:
        line["boundary"] = _pick(bd, "error") or {k: x for k, x in bd.items() if k.endswith("_fps")}
    line["detail"] = DETAIL_NAME
    line = _r(line)
    # never lose the line to its own size: drop the optional parts, least important first
    for k in ("kernels_ms_frac", "boundary", "ingest", "configs", "strong_scan", "e2e10", "roofline_second"):
        if len(json.dumps(line)) < LINE_LIMIT:
            break
        line.pop(k, None)
    return line


def emit(full):
    """detail -> bench_detail.json (next to the script, and gpurun_out/ where that exists) and stderr; the compact line -> stdout, last"""
    line = compact_line(full)
    blob = json.dumps(full, indent=1, default=str)
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        try:
            if os.path.isdir(d):
                with open(os.path.join(d, DETAIL_NAME), "w") as f:
                    f.write(blob + "\n")
        except OSError:
            pass
    print(json.dumps({"bench_detail": full}, default=str), file=sys.stderr, flush=True)
    sys.stdout.flush()
    print(json.dumps(line), flush=True)
    return line


DUMP_LIMIT = 64 << 20                  # bytes of all dumped arrays together
DUMP_SEED = 0x5EED0D0D
DUMP_RECT_FRAMES = 128                 # erased logo rectangles: frames sampled
DUMP_RECORD_FRAMES = 65536             # per-frame records: all frames up to this many, a sample beyond


def dump_sample(n, k):
    """sorted indices of a fixed, seeded sample of k of n frames (all n where k >= n)"""
    if k >= n:
        return np.arange(n)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=k, replace=False))


def dump_outputs(outdir, arrays):
    """arrays: name -> array (numpy or torch).  Written as outdir/<name>.npy: floating point as float32, integers as float64 (the
    integer outputs are sums far below 2**53, so the conversion is exact)"""
    conv = {}
    for name, a in arrays.items():
        if hasattr(a, "detach"):
            a = a.detach().cpu().numpy()
        a = np.asarray(a)
        exact32 = a.dtype.kind == "f" and a.dtype.itemsize <= 4 or a.dtype.kind in "iub" and a.dtype.itemsize <= 2
        conv[name] = np.ascontiguousarray(a, np.float32 if exact32 else np.float64)
    total = sum(a.nbytes for a in conv.values())
    if total > DUMP_LIMIT:
        raise SystemExit(f"--dump-outputs: {total} bytes of outputs exceed the {DUMP_LIMIT}-byte limit")
    os.makedirs(outdir, exist_ok=True)
    for name, a in conv.items():
        np.save(os.path.join(outdir, name + ".npy"), a)


def main():
    args = parse_args()
    if args.dump_outputs and args.workload == "e2e10":
        raise SystemExit("--dump-outputs: available for the headline workload and --scaling strong, not for --workload e2e10")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        respawn_under_torchrun(args)
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert torch.cuda.is_available(), "bench.py needs a GPU (there is no CPU path)"
    # AMT_BENCH_SHARED_GPU=1: every rank on device 0, collectives over gloo -- a dry run of the multi-rank control flow on a 1-GPU box
    # (tests the launcher, the sharding and the exchange steps; its numbers mean nothing)
    shared_gpu = os.environ.get("AMT_BENCH_SHARED_GPU") == "1"
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if shared_gpu:
            local_rank = 0
            dist.init_process_group("gloo")
        else:
            if torch.cuda.device_count() < world:
                raise SystemExit(f"--gpus {world}: only {torch.cuda.device_count()} HIP devices visible (one rank per GPU)")
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        assert dist.get_world_size() == world
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # what the collective backend itself reports, not what the environment asked for: an all_reduce of ones over the device tensors
    # (its sum is the number of ranks the RCCL communicator really joined) and an all_gather of each rank's PCI bus id
    rccl = {"backend": None, "world_size_observed": 1, "distinct_devices": 1}
    if world > 1:
        one = torch.ones(1, device="cpu" if shared_gpu else dev, dtype=torch.int32)
        dist.all_reduce(one)
        ids = [None] * world
        dist.all_gather_object(ids, torch.cuda.get_device_properties(dev).pci_bus_id if hasattr(torch.cuda.get_device_properties(dev), "pci_bus_id")
                               else f"{os.uname().nodename}:{local_rank}")
        rccl = {"backend": ("rccl" if dist.get_backend() == "nccl" else dist.get_backend()), "world_size_observed": int(one.item()),
                "distinct_devices": len(set(ids))}
        if rccl["world_size_observed"] != world:
            raise SystemExit(f"collective backend joined {rccl['world_size_observed']} ranks, WORLD_SIZE says {world}")

    import amt_synth as S
    from amatsukaze_amd import AMTAnalyzeLogo, AMTEraseLogo, Context, DeviceClip, FrameStats, Logo, LogoFrame
    from amatsukaze_amd import sharding as SH

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if world == 1:
            return x
        tt = torch.tensor([x], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item())

    logos_np, alpha, alphaUV = make_logos()
    ctx = Context(local_rank)          # launches on torch's current stream: stream-ordered with the torch copies below
    logos = [Logo.from_planes(ctx, d, LW, LH, W, H, IMGX, IMGY) for d in logos_np]

    # ================================================================================================================
    # BASELINE configs[4]: end-to-end 10-bit stream, frames sharded (tools/bench_e2e.py)
    # ================================================================================================================
    def e2e10():
        import types
        import bench_e2e
        E = types.SimpleNamespace(torch=torch, dist=dist, rank=rank, world=world, dev=dev, ctx=ctx, logos_np=logos_np, alpha=alpha, alphaUV=alphaUV,
                                  fence=fence, max_over_ranks=max_over_ranks, OracleLogos=OracleLogos, maskratio=MASKRATIO)
        # default stream: one GPU's share of the 4-hour stream PER RANK (53 946 frames x world: the whole 431 568-frame stream of configs[4] at
        # N = 8) -- per-GPU work fixed as N grows, i.e. weak scaling; an explicit --e2e-frames fixes the total instead (strong)
        nt = args.e2e_frames or bench_e2e.SHARE_FRAMES * world
        return bench_e2e.run(E, nt=nt, chunk=args.e2e_chunk, verify=not args.no_verify, mode=args.analysis_mode,
                             scaling="strong" if args.e2e_frames else "weak", verify_budget_s=args.e2e_verify_seconds)

    if args.workload == "e2e10":
        r = e2e10()
        if rank == 0:
            if r["verified"]["ok"] is False:
                print(json.dumps({"e2e10": r}), file=sys.stderr, flush=True)
                raise SystemExit("e2e10 verification FAILED: sampled blocks differ from the CPU oracle")
            line = {"metric": "frames/sec 1920x1080i 10-bit logo+CM+KFM end-to-end pass", "value": r["value"], "unit": "frames/sec", "n_gpus": world,
                    "steps": 1, "warmup": 0, "ms_per_step": r["timed_s"] * 1e3, "higher_is_better": True, "scaling": r["scaling"], "vs_baseline": None,
                    "dtype": "f32", "data": "synthetic",
                    "config": {"workload": r["workload"], "frames_total": r["frames_total"], "logo": f"{LW}x{LH}@(1600,64)", "maskratio": MASKRATIO,
                               "analysis_mode": args.analysis_mode, "parallelism": f"frames sharded x{world}"},
                    "collectives": rccl, "e2e10": r}
            # the dominant 16-bit kernel of rank 0's chunk loop (HIP events on the launch stream; traffic from the committed PMC passes)
            r16 = r.get("roofline16") or {}
            if r16:
                dom = max(r16, key=lambda k: r16[k]["total_ms"])
                k = r16[dom]
                line["roofline"] = {"kernel": dom, "bound": k["bound"], "achieved": k["achieved"], "peak": k["peak"], "unit": k["unit"], "frac": k["frac"],
                                    "traffic": (k["traffic_bytes_per_frame"] * r["frames_per_gpu"] / max(1, k["launches"])) if k["traffic_bytes_per_frame"] else None, "traffic_source": k["traffic_source"], "avg_launch_ms": k["total_ms"] / max(1, k["launches"]),
                                    "algorithmic_bytes_per_launch": k["algorithmic_bytes_per_frame"] * r["frames_per_gpu"] / max(1, k["launches"])}
            emit(line)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ================================================================================================================
    # strong scaling: BASELINE configs[3] -- the all-frames LogoFrame scan of a 60-minute stream, frames sharded
    # ================================================================================================================
    def strong_scan(dump=None):
        NT = args.strong_frames
        f0, f1 = SH.shard_range(NT, rank, world)
        nloc = f1 - f0
        t0 = time.perf_counter()
        Yl = S.make_clip_torch(nloc, W, H, 0x5EED0004, alpha, alphaUV, IMGX, IMGY, dev, period=900, fade=12, pitchY=PITCH_Y,
                               start=f0, chroma=False)["Y"]
        torch.cuda.synchronize()
        gen_s = time.perf_counter() - t0
        lf = LogoFrame(ctx, logos, MASKRATIO)
        lf.begin(W, H, 8, NT)
        gathered = [None]

        def sstep():
            lf.scan_batch(Yl, 8, f0, nloc)                            # this rank's frames [f0, f1) of the clip
            if world > 1:
                local = torch.from_numpy(lf.evalResults[f0:f1]).to(dev)
                full = SH.gather_frame_records(local, NT)             # RCCL all_gather of 8 B per frame per logo
                gathered[0] = full
                if rank == 0:
                    lf.set_results(0, full.cpu().numpy())
            if rank == 0:
                lf.selectLogo(len(logos))                             # host decisions over the whole clip (LogoScan.hpp:1647-1682)

        for _ in range(2):
            sstep()
        fence()
        ctx.profile(True)
        t0 = time.perf_counter()
        for _ in range(args.strong_steps):
            sstep()
        fence()
        el = max_over_ranks(time.perf_counter() - t0)
        prof = ctx.profile_report()
        ctx.profile(False)
        if dump and rank == 0:                                        # the last timed step's records (the whole clip's on rank 0) and decision
            rec = lf.evalResults
            sel = dump_sample(NT, DUMP_RECORD_FRAMES)
            dump_outputs(dump, {"scan_records": rec[sel] if len(sel) < NT else rec,
                                "logo_selection": np.array([lf.getBestLogo(), lf.getLogoRatio()], np.float64)})
        # ---- EVERY record of this rank's shard against the CPU oracle (threaded; only the logo rectangle's rows travel to the host):
        #      LogoScan.hpp:1543-1568.  Flags and frame counts are reduced over the ranks. ----
        vall = None
        if not args.no_verify:
            import bench_verify as BV
            ol = OracleLogos(logos_np)
            vr = BV.verify_scan_records(torch, ol, 8, f0, f1, lambda lo, hi: Yl[lo - f0:hi - f0, IMGY:IMGY + LH], lf.evalResults, IMGY,
                                        threads=max(1, BV.host_threads() // (world if shared_gpu or world > 1 else 1)))
            vt = torch.tensor([int(vr["records_equal_oracle"]), vr["frames"]], dtype=torch.int64, device="cpu" if shared_gpu else dev)
            if world > 1:
                vmin = vt.clone(); dist.all_reduce(vmin, op=dist.ReduceOp.MIN)
                dist.all_reduce(vt, op=dist.ReduceOp.SUM)
                vt[0] = vmin[0]
            vall = {"frames": int(vt[1]), "records_equal_oracle": bool(vt[0]), "seconds_rank0": vr["seconds"], "threads_per_rank": vr["threads"]}
            if not vall["records_equal_oracle"]:
                raise SystemExit(f"strong_scan verification FAILED: scan records differ from the CPU oracle ({vr.get('mismatching_chunks')} on rank {rank})")
        out = None
        if rank == 0:
            rec = lf.evalResults                                      # (NT, 3, 2): the whole clip's records on rank 0
            # sharded == unsharded on sampled frames: regenerate blocks that straddle shard boundaries (frames are a function
            # of their absolute index), scan them in one single-GPU launch, compare bytes
            probes = sorted({0, NT - 16} | {max(0, min(NT - 16, SH.shard_range(NT, r, world)[0] - 8)) for r in range(1, world)} |
                            {max(0, min(NT - 16, (NT * k) // 8 - 8)) for k in range(1, 8)})
            lf2 = LogoFrame(ctx, logos, MASKRATIO)
            lf2.begin(W, H, 8, 16)
            same = True
            for p0 in probes:
                Yp = S.make_clip_torch(16, W, H, 0x5EED0004, alpha, alphaUV, IMGX, IMGY, dev, period=900, fade=12, pitchY=PITCH_Y,
                                       start=p0, chroma=False)["Y"]
                lf2.scan_batch(Yp, 8, 0, 16)
                same &= lf2.evalResults.tobytes() == np.ascontiguousarray(rec[p0:p0 + 16]).tobytes()
            if not same:
                raise SystemExit("strong_scan verification FAILED: the sharded records differ from a single-launch scan of the same frames")
            calls, ms = prof.get("logo_eval_pair_kernel.scan", prof.get(EVAL + ".scan", (0, 0.0)))
            out = {"workload": f"BASELINE configs[3]: {NT}-frame (60 min) 1440x1080i Y-only LogoFrame scan, 3 logos, frames sharded "
                               f"over {world} GPU(s) by contiguous range, all_gather of the records, selectLogo on rank 0",
                   "frames_total": NT, "frames_per_gpu": nloc, "n_gpus": world, "steps": args.strong_steps,
                   "value": NT * args.strong_steps / el, "unit": "frames/sec", "ms_per_step": el / args.strong_steps * 1e3,
                   "scaling": "strong", "scan_kernel_ms_rank0": ms / max(1, calls),
                   "records_sha256": hashlib.sha256(np.ascontiguousarray(rec).tobytes()).hexdigest(),
                   "best_logo": lf.getBestLogo(), "logo_ratio": lf.getLogoRatio(),
                   "verified": {"frames": vall["frames"] if vall else 0, "equals_cpu_oracle": vall["records_equal_oracle"] if vall else None,
                                "all_frames": vall, "probe_blocks": len(probes), "sharded_equals_single_launch": bool(same),
                                "how": "every record of every rank's shard against the threaded CPU oracle (bytes); sampled blocks across the "
                                       "shard boundaries against a single-launch scan"},
                   "clip_generation_s": gen_s,
                   "note": "records_sha256 is the hash of all gathered {corr0,corr1} records: identical at every N means the sharded "
                           "scan reproduces the single-GPU scan bit for bit"}
        del Yl
        torch.cuda.empty_cache()
        # ---- the "full LogoScan" of the same configuration: ScanLogo (LogoScan.hpp:917-1079) over the sharded stream -- an all-gather of
        #      per-rank valid counts hands out the numMaxFrames quota in stream order (:885), three exact int64 all-reduces ----
        sl = sharded_scanlogo(ctx, dev, alpha, alphaUV, rank, world, f0, nloc, NT, max_frames=args.scanlogo_max_frames, verify=not args.no_verify)
        if out is not None:
            out["scanlogo"] = sl
        return out

    if args.scaling == "strong":
        ss = strong_scan(dump=args.dump_outputs)
        if rank == 0:
            line = {"metric": "frames/sec 1440x1080i logo+CM+KFM pass", "value": ss["value"], "unit": "frames/sec", "n_gpus": world,
                    "steps": args.strong_steps, "warmup": 2, "ms_per_step": ss["ms_per_step"], "higher_is_better": True,
                    "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                    "config": {"workload": ss["workload"], "frames_total": ss["frames_total"], "logo": f"{LW}x{LH}@({IMGX},{IMGY})",
                               "maskratio": MASKRATIO, "parallelism": f"frames sharded x{world}"},
                    "collectives": rccl, "strong_scan": ss}
            emit(line)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ================================================================================================================
    # the headline pass (BASELINE configs[1]); with N ranks every rank owns its own batch (weak scaling)
    # ================================================================================================================
    N = args.frames
    gen = lambda: S.make_clip_torch(N, W, H, 0x5EED0002 + rank, alpha, alphaUV, IMGX, IMGY, dev, period=900, fade=12,
                                    pitchY=PITCH_Y, pitchUV=PITCH_UV, start=rank * N)
    clip = gen()
    dclip = DeviceClip(clip["Y"], clip["U"], clip["V"], W, H, 8)
    # Device partition: the frame metrics stream bytes (HBM-bound, the vector ALUs a third busy), the logo kernels do arithmetic (no HBM
    # traffic to speak of).  One after the other each leaves half the machine idle; launched together on the whole device they do not
    # co-schedule (the logo kernels take every CU's registers and LDS).  Two contexts on complementary CU ranges run them beside each
    # other: metrics on units [0, M), analysis + scan + erase on [M, ncu).
    NCU = ctx.cu_count()
    MCU = args.metrics_cus if 0 < args.metrics_cus < NCU else 0
    if MCU:
        ctxL, ctxM = Context(local_rank), Context(local_rank)
        sL, sM = ctxL.use_cu_range(MCU, NCU - MCU), ctxM.use_cu_range(0, MCU)
    else:
        ctxL = ctxM = ctx
        sL = sM = None
    lf = LogoFrame(ctxL, logos, MASKRATIO)
    lf.begin(W, H, 8, N)
    analyzer = AMTAnalyzeLogo(ctxL, logos[0], MASKRATIO, mode=args.analysis_mode)
    eraser = AMTEraseLogo(ctxL, logos[0], "", 0, 16)
    stats = FrameStats(ctxM, W, H, 8)
    d_analysis = torch.empty((N, 33), dtype=torch.float32, device=dev)
    d_stats = torch.empty((N, 8), dtype=torch.int64, device=dev)
    h_analysis = torch.empty((N, 33), dtype=torch.float32).pin_memory()
    d_fades = torch.empty((N, 2), dtype=torch.float32, device=dev)
    an_ready = torch.cuda.Event()
    last = {}
    # AMTEraseLogo::GetFrameT takes a writable copy of the frame and rewrites its logo rectangle (LogoScan.hpp:1346-1347).  Default:
    # `wclip` IS that copy -- a second resident batch; Delogo reads dclip and writes wclip's rectangle, so dclip stays what every
    # step analyses.  --erase-in-place (rounds 1-5; always with host-side fades): the erase rewrites dclip itself and the step puts the
    # rectangles back (48 KB per frame, device to device: housekeeping inside the timed region) instead of analysing erased frames.
    to_copy = not args.erase_in_place and args.fades == "device" and not args.no_erase
    wclip = DeviceClip(dclip.Y.clone(), dclip.U.clone(), dclip.V.clone(), W, H, 8) if to_copy else None
    rect = (dclip.Y[:, IMGY:IMGY + LH, IMGX:IMGX + LW].clone(), dclip.U[:, IMGY // 2:(IMGY + LH) // 2, IMGX // 2:(IMGX + LW) // 2].clone(),
            dclip.V[:, IMGY // 2:(IMGY + LH) // 2, IMGX // 2:(IMGX + LW) // 2].clone())

    # 8-byte elements where the geometry allows (pitch, origin and width multiples of 8): the strided copy kernel moves one element
    # per thread, and the restore is housekeeping inside the timed region
    def wide(t, x0, x1):
        if t.stride(1) % 8 == 0 and t.stride(0) % 8 == 0 and x0 % 8 == 0 and x1 % 8 == 0 and t.data_ptr() % 8 == 0 and t.element_size() == 1:
            return t.view(torch.int64), x0 // 8, x1 // 8
        return t, x0, x1
    dst_views = []
    for t, r, (y0, y1, x0, x1) in ((dclip.Y, rect[0], (IMGY, IMGY + LH, IMGX, IMGX + LW)),
                                   (dclip.U, rect[1], (IMGY // 2, (IMGY + LH) // 2, IMGX // 2, (IMGX + LW) // 2)),
                                   (dclip.V, rect[2], (IMGY // 2, (IMGY + LH) // 2, IMGX // 2, (IMGX + LW) // 2))):
        tv, a, b = wide(t, x0, x1)
        dst_views.append((tv[:, y0:y1, a:b], r.view(torch.int64) if tv.dtype == torch.int64 else r))

    def restore_rectangles():
        for dv, sv in dst_views:
            dv.copy_(sv)

    def step(collective=True, restore=True, an=None, in_place=False):
        cur = torch.cuda.current_stream()
        if MCU:                                                      # both partitions start behind what torch's stream did to the frames
            sL.wait_stream(cur)
            sM.wait_stream(cur)
        (an or analyzer).analyze_device(dclip.Y, 8, d_analysis)      # a11: 33 evaluations per frame
        with torch.cuda.stream(sL if MCU else cur):
            h_analysis.copy_(d_analysis, non_blocking=True)          # stream-ordered behind the analysis kernel
            an_ready.record()
        lf.scan_batch(dclip.Y, 8, 0, N)                              # a9: all-frames scan, 3 logos x 2 fades
        stats.run_device(dclip.Y, d_stats)                           # CM field-diff + KFM comb metrics (source frames), on its own CUs
        if MCU:
            sL.wait_stream(sM)                                       # Delogo rewrites what the metrics read
        if not args.no_erase:
            if args.fades == "device":
                eraser.calc_fades_device(d_analysis, N, out=d_fades)     # a12 CalcFade / CalcFade2 on the device: no host round trip
                eraser.erase_device_fades(dclip, d_fades, dst=None if in_place else wclip)     # a12 Delogo: into the writable copy (or in place)
                last["fades"] = None                                     # (read back from d_fades where needed, outside the timed region)
            else:
                an_ready.synchronize()                                   # the host decides while the scan / metrics kernels run
                fades = eraser.calc_fades(h_analysis.numpy(), N)         # a12 CalcFade / CalcFade2
                eraser.erase(dclip, fades)                               # a12 Delogo, in place
                last["fades"] = fades
            if MCU:
                cur.wait_stream(sL)
            if restore and (in_place or not to_copy):
                restore_rectangles()                                 # bench housekeeping (inside the timed region, ~0.4 ms)
        elif MCU:
            cur.wait_stream(sL)
        if world > 1 and collective:
            ev = torch.from_numpy(lf.evalResults).to(dev)
            SH.gather_frame_records(ev, N * world)                   # the scan's one exchange step (RCCL all_gather)

    def profile_on(on):
        for c in {id(ctxL): ctxL, id(ctxM): ctxM}.values():
            c.profile(on)

    def profile_read():
        rep = dict(ctxL.profile_report())
        if ctxM is not ctxL:
            rep.update(ctxM.profile_report())
        return rep

    for _ in range(args.warmup):
        step()
    fence()
    if args.full:                                                    # per-kernel HIP events on the launch stream (the kernel table, roofline)
        profile_on(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    prof = {}
    if args.full:
        prof = profile_read()
        profile_on(False)
    elapsed = max_over_ranks(elapsed)

    # what the last timed step computed, before anything below runs the step again
    if args.dump_outputs and rank == 0:
        rows = dump_sample(N, DUMP_RECORD_FRAMES)
        outs = {"analysis": d_analysis[torch.from_numpy(rows).to(dev)], "scan_records": lf.evalResults[rows],
                "frame_metrics": d_stats[torch.from_numpy(rows).to(dev)]}
        if not args.no_erase:
            outs["fades"] = d_fades[torch.from_numpy(rows).to(dev)] if args.fades == "device" else last["fades"][rows]
        if to_copy:                                                  # the erased frames (the writable copy): the logo rectangle of sampled frames
            sel = torch.from_numpy(dump_sample(N, DUMP_RECT_FRAMES)).to(dev)
            outs["erased_Y_rect"] = wclip.Y[sel, IMGY:IMGY + LH, IMGX:IMGX + LW]
            outs["erased_U_rect"] = wclip.U[sel, IMGY // 2:(IMGY + LH) // 2, IMGX // 2:(IMGX + LW) // 2]
            outs["erased_V_rect"] = wclip.V[sel, IMGY // 2:(IMGY + LH) // 2, IMGX // 2:(IMGX + LW) // 2]
        dump_outputs(args.dump_outputs, outs)

    fps = N * world * args.steps / elapsed
    line = {
        "metric": "frames/sec 1440x1080i logo+CM+KFM pass",
        "value": fps, "unit": "frames/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        # (`workload` must survive the compact line's 120-character cut: the list of passes, no prose)
        "config": {"workload": f"configs[1]: {N}x 1440x1080i 8-bit in HBM: AMTAnalyzeLogo, LogoFrame scan x3, CM/KFM metrics, CalcFade, AMTEraseLogo",
                   "analysis_mode": args.analysis_mode,
                   # the headline is NOT the drop-in default: the library and the plugin's "AMTAnalyzeLogo" evaluate in exact mode (every record
                   # bit-identical); the linear-guarded mode is opt-in (amtgpu_analyze_set_mode / AMTAnalyzeLogoFast).  exact_mode.value is
                   # the same step at the default
                   "library_default_mode": "exact",
                   "value_is_in_mode": ("linear-guarded (opt-in; identical fades and erased frames, scores within 1e-4): see exact_mode.value for the library default"
                                        if args.analysis_mode == "linear" else "exact (the library default)"),
                   "calc_fade": args.fades,
                   "erase": ("none" if args.no_erase else "into a resident writable copy (MakeWritable's frame)" if to_copy else
                             "in place, rectangles put back inside the step"),
                   "device_partition": ({"metrics_cus": MCU, "logo_cus": NCU - MCU, "how": "two contexts on CU-range streams (amtgpu_stream_create_cu_range): the "
                                         "frame metrics run beside the analysis + scan; erase waits for both"} if MCU else None),
                   "frames_per_gpu": N, "logo": f"{LW}x{LH}@({IMGX},{IMGY})", "maskratio": MASKRATIO,
                   "parallelism": f"frames sharded x{world} (one private batch per rank)" if world > 1 else "single GPU"},
        "timed_region_s": elapsed, "collectives": rccl,
    }
    if not args.full:
        if rank == 0:
            emit(line)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    if not args.no_erase and last.get("fades") is None:
        last["fades"] = d_fades.cpu().numpy()

    # ---- the same pass with the exact (bit-identical records) analysis, for the record next to the headline ----
    exact_mode = None
    if args.analysis_mode == "linear" and args.exact_steps > 0 and not args.no_alt_mode:
        an_exact = AMTAnalyzeLogo(ctxL, logos[0], MASKRATIO, mode="exact")
        step(an=an_exact)
        fence()
        t0 = time.perf_counter()
        for _ in range(args.exact_steps):
            step(an=an_exact)
        fence()
        el_x = max_over_ranks(time.perf_counter() - t0)
        exact_mode = {"value": N * world * args.exact_steps / el_x, "unit": "frames/sec", "ms_per_step": el_x / args.exact_steps * 1e3,
                      "steps": args.exact_steps, "what": "the same step with AMTAnalyzeLogo in exact mode (the library default): every analysis "
                                                         "record bit-identical to the reference's, not just the decisions"}
        del an_exact
    # ---- and with rounds 1-5's erase (in place, rectangles put back inside the step), for the record ----
    in_place_step = None
    if to_copy and args.exact_steps > 0 and not args.no_alt_mode:
        step(in_place=True)
        fence()
        t0 = time.perf_counter()
        for _ in range(args.exact_steps):
            step(in_place=True)
        fence()
        el_p = max_over_ranks(time.perf_counter() - t0)
        in_place_step = {"value": N * world * args.exact_steps / el_p, "unit": "frames/sec", "ms_per_step": el_p / args.exact_steps * 1e3,
                         "steps": args.exact_steps, "what": "the headline's step with AMTEraseLogo rewriting the analysed frames in place and the rectangles "
                                                            "put back inside the timed region (rounds 1-5's step; --erase-in-place)"}

    # ---- where a step's wall time goes (untimed): the same calls once more, fenced one by one ----
    phases = None
    if rank == 0 and not args.no_erase:
        def timed(fn):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3, r
        phases = {}
        phases["analysis"], _ = timed(lambda: analyzer.analyze_device(dclip.Y, 8, d_analysis))
        phases["analysis_records_to_host"], _ = timed(lambda: h_analysis.copy_(d_analysis, non_blocking=True))
        phases["scan"], _ = timed(lambda: lf.scan_batch(dclip.Y, 8, 0, N))
        phases["frame_metrics"], _ = timed(lambda: stats.run_device(dclip.Y, d_stats))
        phases["host_calc_fades"], fd = timed(lambda: eraser.calc_fades(h_analysis.numpy(), N))
        phases["device_calc_fades"], _ = timed(lambda: eraser.calc_fades_device(d_analysis, N, out=d_fades))
        if to_copy:
            phases["erase_into_the_writable_copy"], _ = timed(lambda: eraser.erase_device_fades(dclip, d_fades, dst=wclip))
        else:
            phases["erase"], _ = timed(lambda: eraser.erase(dclip, fd))
            phases["restore_rectangles_bench_housekeeping"], _ = timed(restore_rectangles)
        phases = {k: round(v, 3) for k, v in phases.items()}
        phases["note"] = ("each call fenced with a device synchronise (so launch latency is inside every figure); the timed steps use "
                          + ("the device CalcFade: the whole step is stream-ordered, the host only enqueues" if args.fades == "device" else
                             "the host CalcFade, overlapped with the scan and the frame metrics"))

    # ---- verification (untimed): fresh frames, one more step at the same launch geometry, EVERY frame against the CPU oracle ----
    verified = None
    if not args.no_verify and rank == 0:
        import bench_verify as BV
        del clip
        clip = gen()                                                 # stays resident: the pristine frames the oracle is fed
        dclip.Y.copy_(clip["Y"]); dclip.U.copy_(clip["U"]); dclip.V.copy_(clip["V"])
        if to_copy:
            wclip.Y.copy_(clip["Y"]); wclip.U.copy_(clip["U"]); wclip.V.copy_(clip["V"])
        eclip = wclip if to_copy else dclip                          # where the erased frames are
        d_exact = None
        if args.analysis_mode == "linear":
            # the whole batch through the exact kernel (bit-identical to the reference) BEFORE the step erases the frames: the
            # reference every one of the step's 330 000 linear-guarded scores and 10 000 fade pairs is held against below
            exact_an = AMTAnalyzeLogo(ctx, logos[0], MASKRATIO, mode="exact")
            d_exact = torch.empty((N, 33), dtype=torch.float32, device=dev)
            exact_an.analyze_device(dclip.Y, 8, d_exact)
            torch.cuda.synchronize()
            del exact_an
        step(collective=False, restore=False)                        # rank 0 alone; the erased frames are what gets checked
        torch.cuda.synchronize()
        if not args.no_erase and last.get("fades") is None:
            last["fades"] = d_fades.cpu().numpy()
            # the device decision against the host routine on the same records (bytes, every frame)
            if eraser.calc_fades(h_analysis.numpy(), N).tobytes() != last["fades"].tobytes():
                raise SystemExit("bench verification FAILED: amtgpu_erase_calc_fades_device differs from the host CalcFade")
        # all N frames: scan records, frame metrics, fades and the erased planes as bytes, analysis records as bytes (exact mode) or
        # within 1e-4 (linear-guarded); the oracle on every host core (tools/bench_verify.py)
        verified = BV.verify_range(torch, OracleLogos(logos_np), 8, N, 0, N,
                                   lambda lo, hi: (clip["Y"][lo:hi], clip["U"][lo:hi], clip["V"][lo:hi]),
                                   lambda lo, hi: (eclip.Y[lo:hi], eclip.U[lo:hi], eclip.V[lo:hi]),
                                   lf.evalResults, h_analysis.numpy(), last.get("fades"), d_stats.cpu().numpy().astype(np.uint64),
                                   tol=1e-4 if args.analysis_mode == "linear" else 0.0, erase=not args.no_erase)
        if to_copy and not (torch.equal(dclip.Y, clip["Y"]) and torch.equal(dclip.U, clip["U"]) and torch.equal(dclip.V, clip["V"])):
            raise SystemExit("bench verification FAILED: the erase into the writable copy touched its source frames")
        del clip
        verified["analysis_mode"] = args.analysis_mode
        verified["analysis_compare"] = ("bytes" if args.analysis_mode == "exact" else
                                        "every frame vs the CPU oracle: abs <= 1e-4 (fades and erased frames: bytes); and vs the exact GPU "
                                        "kernel: analysis_max_abs / analysis_max_rel / fades_equal_all")
        verified["guard_refined_frames"] = analyzer.last_refined()
        if d_exact is not None:
            verified.update(tolerance_accounting(h_analysis.numpy(), d_exact.cpu().numpy(), last["fades"], eraser, analyzer, N))
            del d_exact
        if args.analysis_mode == "linear" and verified["guard_refined_frames"] > N // 20:
            # the guard re-evaluates close calls; if it has to redo a large share of the batch the linear kernel itself is off
            # (its errors would be masked by the exact re-evaluation and paid for in time)
            verified["ok"] = False
            verified["guard_overused"] = True
        if not verified.get("tolerance_ok", True):
            verified["ok"] = False
        if not verified["ok"]:
            print(json.dumps({"verified": verified}), file=sys.stderr, flush=True)
            raise SystemExit("bench verification FAILED: the timed configuration's outputs differ from the CPU oracle")
    if world > 1:
        dist.barrier()

    # the other analysis mode, for the record (outside the timed region): the same 10 000-frame launch
    alt_prof = {}
    if rank == 0 and not args.no_alt_mode:
        alt = AMTAnalyzeLogo(ctx, logos[0], MASKRATIO, mode="exact" if args.analysis_mode == "linear" else "linear")
        alt.analyze_device(dclip.Y, 8, d_analysis)
        torch.cuda.synchronize()
        ctx.profile(True)
        for _ in range(5):
            alt.analyze_device(dclip.Y, 8, d_analysis)
        torch.cuda.synchronize()
        alt_prof = ctx.profile_report()
        ctx.profile(False)
        del alt
    if world > 1:
        dist.barrier()

    # free the batch before the attached measurements
    d_fades_host = d_fades.cpu().numpy()
    del d_fades
    if MCU:
        torch.cuda.synchronize()
    del dclip, lf, analyzer, eraser, stats, d_analysis, d_stats, dst_views, rect
    if MCU:
        del sL, sM
        ctxL.close()
        ctxM.close()
    torch.cuda.empty_cache()

    strong = None
    if not args.no_strong:
        try:
            strong = strong_scan()
        except SystemExit:
            raise
        except Exception as e:                                       # e.g. not enough HBM next to another tenant: never lose the line
            strong = {"error": f"{type(e).__name__}: {e}"} if rank == 0 else None

    configs = None
    if rank == 0 and world == 1 and not args.no_configs:
        configs = {}
        for name, fn in (("kfm_1080p_mixed_cadence", config_kfm), ("tenbit_1080p_step", config_tenbit), ("scanlogo_60min", config_scanlogo)):
            try:
                configs[name] = fn(ctx, dev, logos_np, alpha, alphaUV, args)
            except SystemExit:
                raise
            except Exception as e:                                   # never lose the line to an attached measurement
                configs[name] = {"error": f"{type(e).__name__}: {e}"}
            torch.cuda.empty_cache()

    # BASELINE configs[4] end to end, strong-sharded over the ranks of this run (every rank takes part; the same stream at every N)
    e2e = None
    if not args.no_e2e and not args.no_configs:
        try:
            e2e = e2e10()
        except SystemExit:
            raise
        except Exception as e:
            e2e = {"error": f"{type(e).__name__}: {e}"} if rank == 0 else None
        if rank == 0 and e2e and e2e.get("verified", {}).get("ok") is False:
            print(json.dumps({"e2e10": e2e}), file=sys.stderr, flush=True)
            raise SystemExit("e2e10 verification FAILED: sampled blocks differ from the CPU oracle")
        torch.cuda.empty_cache()

    boundary = None
    if rank == 0 and world == 1 and not args.no_configs:
        try:
            boundary = measure_boundary(ctx, logos, local_rank)
        except Exception as e:
            boundary = {"error": f"{type(e).__name__}: {e}"}

    ingest = None
    if rank == 0 and world == 1 and not args.no_ingest:
        try:
            ingest = measure_ingest(ctx, logos, alpha, alphaUV, dev)
        except Exception as e:
            ingest = {"error": f"{type(e).__name__}: {e}"}

    if rank == 0:
        # ---- per-kernel figures (HIP events on the launch stream, inside the timed steps) ----
        an_tab = [logos[0].mask_tables(k, MASKRATIO)["count"] for k in (0, 1, 2)]
        scan_tab = [l.mask_tables(0, MASKRATIO)["count"] for l in logos]
        # algorithmic work per frame (the reference's own operation count) and bytes
        flops_an = FLOPS_PER_MASK_PIXEL * 11 * sum(an_tab) + FLOPS_PER_RECT_PIXEL * 11 * (LW * LH + 2 * LW * (LH // 2))
        flops_scan = FLOPS_PER_MASK_PIXEL * 2 * sum(scan_tab) + FLOPS_PER_RECT_PIXEL * 2 * 3 * LW * LH
        VALU = {"logo_eval_fused_kernel.analysis": (flops_an, LW * LH + 132, "every fade in the reference's fp32 order (bit-exact records)"),
                "logo_eval_linear_kernel.analysis": (flops_an, LW * LH + 132, "all 11 fades from one window evaluation of s and of bg; flops are the "
                                                     "ALGORITHMIC count of the reference (the kernel issues ~4x fewer), so this fraction may pass 0.5"),
                "logo_eval_fused_kernel.scan": (flops_scan, 3 * LW * LH + 24, "3 logos x fades {0,1}, reference order (bit-exact records)"),
                "logo_eval_pair_kernel.scan": (flops_scan, 3 * LW * LH + 24, "3 logos x fades {0,1}: the window of s and the window of bg as the two halves "
                                               "of one packed instruction stream, reference order (bit-exact records)")}
        HBM = {"frame_stats_kernel": W * H, "delogo_kernel": 2 * (LW * LH + 2 * (LW // 2) * (LH // 2))}
        pmc = {}
        try:
            pmc = json.load(open(os.path.join(ROOT, PMC_TRAFFIC)))
        except Exception:
            pass

        if "fades" in last and last["fades"] is None:
            last["fades"] = d_fades_host
        erased_share = float((np.abs(last["fades"]).sum(axis=1) != 0).mean()) if "fades" in last else 1.0

        def kernel_entry(name, calls, ms, frames_per_call, timed, cus):
            e = {"avg_ms": ms / max(1, calls), "launches": calls, "inside_timed_region": timed, "cus": cus}
            fr = frames_per_call * calls
            tr = pmc.get(name, {}).get("hbm_bytes_per_frame")
            if name in VALU:
                fl, ab, what = VALU[name]
                e.update({"bound": "fp32-valu", "achieved_tflops": fl * fr / (ms * 1e-3) / 1e12,
                          "frac_fp32_peak": fl * fr / (ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS,
                          "frac_of_its_cus_peak": fl * fr / (ms * 1e-3) / 1e12 / (FP32_PEAK_TFLOPS * cus / NCU), "flops_per_launch": fl * frames_per_call,
                          "algorithmic_bytes_per_launch": ab * frames_per_call, "hbm_gbs_algorithmic": ab * fr / (ms * 1e-3) / 1e9, "what": what})
            elif name in HBM:
                # Delogo with fade 0 is an identity the kernel skips (no traffic): only frames with a non-zero fade count
                share = erased_share if name == "delogo_kernel" else 1.0
                e.update({"bound": "hbm", "achieved_gbs": HBM[name] * share * fr / (ms * 1e-3) / 1e9,
                          "frac": HBM[name] * share * fr / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                          "algorithmic_bytes_per_launch": HBM[name] * share * frames_per_call})
                if name == "delogo_kernel":
                    e["frames_with_nonzero_fade_share"] = share
            e["hbm_bytes_per_launch_pmc"] = tr * frames_per_call if tr else None
            return e

        out_kern = {name: kernel_entry(name, calls, ms, N, True, (MCU if name == "frame_stats_kernel" else NCU - MCU) if MCU else NCU)
                    for name, (calls, ms) in prof.items() if calls}
        for name, (calls, ms) in alt_prof.items():
            if calls and name not in out_kern:
                out_kern[name] = kernel_entry(name, calls, ms, N, False, NCU)
        timed = {n: e for n, e in out_kern.items() if e["inside_timed_region"] and "bound" in e}
        # the dominant kernel: the longest on the step's critical path.  With the device partitioned the frame metrics run beside the logo
        # kernels on their own units and end before them (roofline_second describes them)
        on_path = {n: e for n, e in timed.items() if not (MCU and n == "frame_stats_kernel")}
        order = sorted(on_path, key=lambda n: -on_path[n]["avg_ms"] * on_path[n]["launches"]) + (["frame_stats_kernel"] if MCU and "frame_stats_kernel" in timed else [])

        def roofline_of(dom):
            kk = timed[dom]
            src = (PMC_TRAFFIC + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this bench's own launches, tools/gpu_prof_bench.sh; not "
                   "collected inside the timed run)") if kk["hbm_bytes_per_launch_pmc"] else None
            part = ({"cus": kk["cus"], "device_cus": NCU,
                     "partition": f"the device is partitioned ({MCU} units stream the frame metrics, {NCU - MCU} run the logo kernels beside them): this kernel "
                                  f"ran on {kk['cus']} of {NCU} units"} if MCU else {})
            if kk.get("bound") == "fp32-valu":
                # `peak` = the fp32 vector peak of the units the kernel ran on; the whole device's peak and the fraction of it are beside it
                return {"kernel": dom, "bound": "fp32-valu", "achieved": kk["achieved_tflops"], "peak": FP32_PEAK_TFLOPS * kk["cus"] / NCU, "unit": "TFLOP/s",
                        "frac": kk["frac_of_its_cus_peak"], "peak_whole_device": FP32_PEAK_TFLOPS, "frac_whole_device": kk["frac_fp32_peak"], **part,
                        "traffic": kk["hbm_bytes_per_launch_pmc"], "traffic_source": src,
                        "avg_launch_ms": kk["avg_ms"], "flops_per_launch": kk["flops_per_launch"],
                        "algorithmic_bytes_per_launch": kk["algorithmic_bytes_per_launch"],
                        "note": "fp32 VALU kernel (no MFMA: per-pixel private 25-tap kernels, no operand reuse); priced against the fp32 "
                                "vector peak with FMA counted as 2; flops are the reference's own operation count (101 per mask-pixel "
                                "evaluation + 6 per rectangle pixel per evaluation); the exact kernels use mul/add/sub without FMA "
                                "contraction (bit-exactness), so 0.5 is their ceiling. " + kk.get("what", "")}
            return {"kernel": dom, "bound": "hbm", "achieved": kk["achieved_gbs"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": kk["frac"], **part,
                    "traffic": kk["hbm_bytes_per_launch_pmc"], "traffic_source": src, "avg_launch_ms": kk["avg_ms"],
                    "algorithmic_bytes_per_launch": kk["algorithmic_bytes_per_launch"],
                    **({"note": "on its partition the kernel is bound by what a compute unit streams (~39 GB/s per unit: vector ALU and bytes in flight, "
                                "profiles/r04_notes.md), not by HBM; it ends before the logo kernels it runs beside"} if MCU else {})}

        # the dominant kernel of the timed steps; the runner-up beside it (the linear analysis and the exact scan take about the same
        # time per step, and the linear kernel's fraction prices the reference's operation count, not what it issues)
        roofline = roofline_of(order[0]) if order else None
        roofline_second = roofline_of(order[1]) if len(order) > 1 else None
        cpu = None
        if args.cpu_frames > 0 and world == 1:        # the CPU baseline is reported at N=1 only
            cpu = cpu_baseline(args.cpu_frames, logos_np, alpha, alphaUV, args.cpu_seconds)
        line.update({
            "step_phases_ms": phases,
            "roofline": roofline, "roofline_second": roofline_second, "cpu_baseline": cpu,
            "gpu_over_cpu": (fps / cpu["value"]) if cpu else None,
            "gpu_over_cpu_all_cores": (fps / cpu["all_cores"]["value"]) if cpu else None,
            "exact_mode": exact_mode, "in_place_erase_step": in_place_step,
            "verified": verified, "configs": configs, "e2e10": e2e, "boundary": boundary, "strong_scan": strong, "ingest": ingest,
            "kernels": out_kern,
        })
        emit(line)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()



# --------------------------------------------------------------------------------------------------------------------
# attached measurements of the other BASELINE configurations (rank 0, N = 1; outside the timed region of the headline)
# --------------------------------------------------------------------------------------------------------------------
def _prof(ctx, fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ctx.profile(True)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / reps
    rep = ctx.profile_report()
    ctx.profile(False)
    return wall, {k: ms / max(1, c) for k, (c, ms) in rep.items() if c}


def config_kfm(ctx, dev, logos_np, alpha, alphaUV, args, N=18000, SEG=1800):
    """BASELINE configs[2]: KFM/CM whole-frame pass on 18 000 frames (10 min) of 1920x1080 8-bit whose cadence alternates 24p / 30i /
    30p every 1 800 frames and whose scene changes every 97 frames (the generator's own labels are the ground truth the detectors
    are held against).  SELF-SPECIFIED passes: parity unpinned."""
    import torch
    import amt_synth as S
    if os.path.join(ROOT, "oracle") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import frame_stats_oracle as FS                                  # the checker of the self-specified passes (numpy)
    from amatsukaze_amd import FrameStats
    Wk, Hk = 1920, 1080
    order = ("24p", "30i", "30p")
    code = {"30i": 0, "24p": 1, "30p": 2}
    Y = torch.empty((N, Hk, Wk), dtype=torch.uint8, device=dev)
    truth = np.zeros(N, np.uint8)
    t0 = time.perf_counter()
    for k, s0 in enumerate(range(0, N, SEG)):
        n = min(SEG, N - s0)
        cad = order[k % 3]
        Y[s0:s0 + n] = S.make_clip_torch(n, Wk, Hk, 0x5EED0003, None, None, 0, 0, dev, cadence=cad, start=s0, chroma=False, noise="soft")["Y"]
        truth[s0:s0 + n] = code[cad]
    torch.cuda.synchronize()
    gen_s = time.perf_counter() - t0
    fs = FrameStats(ctx, Wk, Hk, 8)
    out = torch.zeros((N, 8), dtype=torch.int64, device=dev)
    wall, kern = _prof(ctx, lambda: fs.run_device(Y, out), 5)
    m = out.cpu().numpy().astype(np.uint64)
    t0 = time.perf_counter()
    cad, ph = fs.cadence(m)
    sc = fs.scene_changes(m)
    host_ms = (time.perf_counter() - t0) * 1e3
    # ---- the kernel against the numpy oracle (bytes) on probe blocks and against the C oracle on EVERY frame; the host decisions against
    #      the oracle's on all metrics ----
    ok_metrics = True
    for b0 in (0, SEG - 12, 2 * SEG - 12, N // 2, N - 24):
        blk = Y[max(0, b0 - 1):b0 + 24].cpu().numpy()
        want = FS.frame_metrics(blk)
        ok_metrics &= bool(np.array_equal(m[b0:b0 + 24], want[(1 if b0 > 0 else 0):]))
    vm = None
    if not args.no_verify:
        import bench_verify as BV
        from amtlib import Oracle
        vm = BV.verify_metrics(torch, Oracle().lib, 8, Wk, Hk, N, lambda lo, hi: Y[lo:hi], m)
        ok_metrics &= vm["metrics_equal_oracle"]
    ocad, oph = FS.classify_cadence(m, Wk, Hk)
    ok_dec = bool(np.array_equal(cad, ocad) and np.array_equal(ph, oph) and sc.tolist() == FS.scene_changes(m, Wk, Hk))
    if not (ok_metrics and ok_dec):
        raise SystemExit(f"configs[2] verification FAILED: metrics == oracle: {ok_metrics}, decisions == oracle: {ok_dec}")
    # ---- detector accuracy against the generator's labels ----
    # interior = frames whose whole 10-frame classifier window [n-4, n+6) lies inside one cadence segment (and inside the clip)
    interior = np.zeros(N, bool)
    for s0 in range(0, N, SEG):
        interior[s0 + 4:max(s0 + 4, min(N, s0 + SEG) - 5)] = True
    agree = cad == truth
    per_class = {c: float(agree[truth == v].mean()) for c, v in code.items()}
    cuts = set(range(97, N, 97))
    det = set(int(x) for x in sc.tolist())
    near = lambda a, B: any((a + d) in B for d in (-1, 0, 1))
    # the interior misses, looked at: where they are relative to the scene cuts and what the per-frame field-match codes were
    c0m, c1m = m[:, 3].astype(np.float64), m[:, 4].astype(np.float64)
    fcode = np.where(c0m * 3 < c1m * 2, "C", np.where(c1m * 3 < c0m * 2, "P", "B"))
    miss = np.nonzero(~agree & interior)[0]
    runs = []
    for n in miss.tolist():
        if runs and n == runs[-1][1] + 1:
            runs[-1][1] = n
        else:
            runs.append([n, n])
    miss_runs = [{"frames": [a, b], "truth": int(truth[a]), "got": sorted(set(int(x) for x in cad[a:b + 1])), "nearest_cut_distance": int(min(abs(a - c) for c in cuts)),
                  "codes_window": "".join(fcode[max(0, a - 4):b + 7].tolist())} for a, b in runs[:40]]
    tp = len(det & cuts)
    acc = {"cadence_agreement_all_frames": float(agree.mean()), "cadence_agreement_segment_interiors": float(agree[interior].mean()),
           "cadence_agreement_per_class": per_class,
           "interior_miss_frames": int(miss.size), "interior_miss_runs": miss_runs,
           "scene_cuts_truth": len(cuts), "scene_cuts_detected": len(det),
           "scene_cut_precision": tp / max(1, len(det)), "scene_cut_recall": tp / max(1, len(cuts)),
           "scene_cut_precision_pm1": sum(near(a, cuts) for a in det) / max(1, len(det)),
           "scene_cut_recall_pm1": sum(near(a, det) for a in cuts) / max(1, len(cuts)),
           "labels": "generator: cadence per 1 800-frame segment (24p = 3:2 pulldown of 23.976p, 30i = fields from consecutive times, 30p); "
                     "cuts where the scene index n // 97 changes"}
    k_ms = kern.get("frame_stats_kernel", wall * 1e3)
    byts = Wk * Hk
    return {"workload": f"BASELINE configs[2]: {N}-frame 1920x1080i 8-bit, cadence 24p/30i/30p alternating every {SEG} frames; whole-frame "
                        "field-difference / combing metrics on the GPU, cadence + scene-change decisions on the host",
            "frames": N, "value": N / wall, "unit": "frames/sec", "ms_per_pass": wall * 1e3, "host_decisions_ms": host_ms,
            "kernels": {"frame_stats_kernel": {"avg_ms": k_ms, "bound": "hbm", "achieved_gbs": byts * N / (k_ms * 1e-3) / 1e9,
                                               "frac": byts * N / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "algorithmic_bytes_per_launch": byts * N}},
            "verified": {"metrics_equal_oracle_on_probe_blocks": ok_metrics, "frames": vm["frames"] if vm else 120, "all_frames": vm,
                         "decisions_equal_oracle": ok_dec, "parity": "unpinned (self-specified pass)"},
            "accuracy_vs_generator_labels": acc, "clip_generation_s": gen_s}


def config_tenbit(ctx, dev, logos_np, alpha, alphaUV, args, N=3000):
    """The 10-bit format of BASELINE configs[4] on one GPU: 1920x1080 YUV420P10 in 16-bit containers, the same step as the
    headline (AMTAnalyzeLogo linear-guarded + LogoFrame scan of 3 logos + frame metrics + CalcFade + AMTEraseLogo)."""
    import torch
    import amt_synth as S
    from amatsukaze_amd import AMTAnalyzeLogo, AMTEraseLogo, DeviceClip, FrameStats, Logo, LogoFrame
    Wk, Hk, X, Y0, bits = 1920, 1080, 1600, 64, 10
    gen = lambda: S.make_clip_torch(N, Wk, Hk, 0x5EED0005, alpha, alphaUV, X, Y0, dev, bits=bits, period=300, fade=12)
    clip = gen()
    dclip = DeviceClip(clip["Y"], clip["U"], clip["V"], Wk, Hk, bits)
    logos = [Logo.from_planes(ctx, d, LW, LH, Wk, Hk, X, Y0) for d in logos_np]
    lf = LogoFrame(ctx, logos, MASKRATIO)
    lf.begin(Wk, Hk, bits, N)
    an = AMTAnalyzeLogo(ctx, logos[0], MASKRATIO, mode=args.analysis_mode)
    er = AMTEraseLogo(ctx, logos[0], "", 0, 16)
    st = FrameStats(ctx, Wk, Hk, bits)
    d_an = torch.empty((N, 33), dtype=torch.float32, device=dev)
    d_st = torch.empty((N, 8), dtype=torch.int64, device=dev)
    rects = [(p, p[:, y0:y1, x0:x1].clone(), (y0, y1, x0, x1)) for p, (y0, y1, x0, x1) in
             ((dclip.Y, (Y0, Y0 + LH, X, X + LW)), (dclip.U, (Y0 // 2, (Y0 + LH) // 2, X // 2, (X + LW) // 2)),
              (dclip.V, (Y0 // 2, (Y0 + LH) // 2, X // 2, (X + LW) // 2)))]
    last = {}

    def step(restore=True):
        an.analyze_device(dclip.Y, bits, d_an)
        lf.scan_batch(dclip.Y, bits, 0, N)
        st.run_device(dclip.Y, d_st)
        rec = d_an.cpu().numpy()
        fades = er.calc_fades(rec, N)
        er.erase(dclip, fades)
        last["fades"], last["an"] = fades, rec
        if restore:
            for pl, keep, (y0, y1, x0, x1) in rects:
                pl[:, y0:y1, x0:x1] = keep

    wall, kern = _prof(ctx, step, 5)
    # ---- verification: fresh frames, one step, EVERY frame against the CPU oracle (bytes; analysis within 1e-4 in linear mode) ----
    verified = None
    if not args.no_verify:
        import bench_verify as BV
        del clip
        clip = gen()                                                  # stays resident: the pristine frames the oracle is fed
        dclip.Y.copy_(clip["Y"]); dclip.U.copy_(clip["U"]); dclip.V.copy_(clip["V"])
        step(restore=False)
        torch.cuda.synchronize()
        verified = BV.verify_range(torch, OracleLogos(logos_np, Wk, Hk, X, Y0, bits), bits, N, 0, N,
                                   lambda lo, hi: (clip["Y"][lo:hi], clip["U"][lo:hi], clip["V"][lo:hi]),
                                   lambda lo, hi: (dclip.Y[lo:hi], dclip.U[lo:hi], dclip.V[lo:hi]),
                                   lf.evalResults, last["an"], last["fades"], d_st.cpu().numpy().astype(np.uint64),
                                   tol=1e-4 if args.analysis_mode == "linear" else 0.0, chunk=256)
        del clip
        verified["guard_refined_frames"] = an.last_refined()
        if not verified["ok"]:
            print(json.dumps({"tenbit_verified": verified}), file=sys.stderr, flush=True)
            raise SystemExit("10-bit configuration: outputs differ from the CPU oracle")
    an_tab = [logos[0].mask_tables(k, MASKRATIO)["count"] for k in (0, 1, 2)]
    scan_tab = [l.mask_tables(0, MASKRATIO)["count"] for l in logos]
    fl_an = FLOPS_PER_MASK_PIXEL * 11 * sum(an_tab) + FLOPS_PER_RECT_PIXEL * 11 * (LW * LH + 2 * LW * (LH // 2))
    fl_sc = FLOPS_PER_MASK_PIXEL * 2 * sum(scan_tab) + FLOPS_PER_RECT_PIXEL * 2 * 3 * LW * LH
    kk = {}
    for name, ms in kern.items():
        e = {"avg_ms": ms}
        if "analysis" in name and "refine" not in name and "eval" in name:
            e.update({"bound": "fp32-valu", "frac_fp32_peak": fl_an * N / (ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, "algorithmic_bytes_per_launch": (2 * LW * LH + 132) * N})
        elif name.endswith(".scan"):
            e.update({"bound": "fp32-valu", "frac_fp32_peak": fl_sc * N / (ms * 1e-3) / 1e12 / FP32_PEAK_TFLOPS, "algorithmic_bytes_per_launch": (3 * 2 * LW * LH + 24) * N})
        elif name == "frame_stats_kernel":
            e.update({"bound": "hbm", "achieved_gbs": 2 * Wk * Hk * N / (ms * 1e-3) / 1e9, "frac": 2 * Wk * Hk * N / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                      "algorithmic_bytes_per_launch": 2 * Wk * Hk * N})
        kk[name] = e
    return {"workload": f"the 10-bit format of BASELINE configs[4] on one GPU: {N}-frame 1920x1080 YUV420P10 (16-bit containers) resident in HBM; the "
                        "headline's step (analysis + scan of 3 logos + frame metrics + CalcFade + erase, rectangles restored)",
            "frames": N, "bits": bits, "analysis_mode": args.analysis_mode, "value": N / wall, "unit": "frames/sec", "ms_per_step": wall * 1e3,
            "kernels": kk, "verified": verified,
            "note": "ms_per_step here includes a synchronous copy of the analysis records to the host (the headline overlaps it)"}


class _DevPtr:
    """a device address that is not a tensor's first byte (amatsukaze_amd.api._p only asks for data_ptr())"""

    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr


_ORACLE_LGD = {}


def scanlogo_oracle_lgd(dev, alpha, alphaUV, NT, max_frames, clip=None, chunk=8192):
    """The CPU oracle's ScanLogo (orc_scanlogo_mt: LogoScan.hpp:794-1080, the ReMakeLogo rounds' per-frame evaluations dealt over the host's
    cores, quota and accumulations in stream order) over the WHOLE configs[3] stream -> the .lgd bytes it writes.  Only the logo rectangle
    of every frame travels to the host (49 152 B per frame).  clip: the resident rect_rows clip of frames [0, NT) if the caller has one,
    else the frames are regenerated here (they are a function of their absolute index).  Cached per (NT, max_frames) in this process."""
    import tempfile
    import torch
    import amt_synth as S
    import bench_verify as BV
    from amtlib import Oracle
    key = (NT, max_frames)
    if key in _ORACLE_LGD:
        return _ORACLE_LGD[key]
    t0 = time.perf_counter()
    hY = np.empty((NT, LH, LW), np.uint8)
    hU = np.empty((NT, LH // 2, LW // 2), np.uint8)
    hV = np.empty_like(hU)
    for c0 in range(0, NT, chunk):
        c1 = min(NT, c0 + chunk)
        c = ({k: clip[k][c0:c1] for k in "YUV"} if clip is not None else
             S.make_clip_torch(c1 - c0, W, H, 0x5EED0004, alpha, alphaUV, IMGX, IMGY, dev, period=900, fade=12, pitchY=PITCH_Y, pitchUV=PITCH_UV,
                               start=c0, rows=(IMGY, IMGY + LH), flat_every=SCANLOGO_FLAT_EVERY))
        hY[c0:c1] = c["Y"][:, :, IMGX:IMGX + LW].cpu().numpy()
        hU[c0:c1] = c["U"][:, :, IMGX // 2:(IMGX + LW) // 2].cpu().numpy()
        hV[c0:c1] = c["V"][:, :, IMGX // 2:(IMGX + LW) // 2].cpu().numpy()
        del c
    t1 = time.perf_counter()
    orc = Oracle()
    nvalid, nread = C.c_int(), C.c_int()
    T = BV.host_threads()
    # the oracle addresses the rectangle as plane + scanx + scany * pitch (LogoScan.hpp:888-893): hand it the address a full plane of pitch
    # LW would start at (never dereferenced outside the rectangle)
    lo = orc.lib.orc_scanlogo_mt(C.c_void_p(hY.ctypes.data - (IMGX + IMGY * LW)), C.c_void_p(hU.ctypes.data - (IMGX // 2 + (IMGY // 2) * (LW // 2))),
                                 C.c_void_p(hV.ctypes.data - (IMGX // 2 + (IMGY // 2) * (LW // 2))), LW * LH, (LW // 2) * (LH // 2), LW, LW // 2,
                                 W, H, NT, IMGX, IMGY, LW, LH, 12, max_frames, 1, C.byref(nvalid), None, T, C.byref(nread))
    if not lo:
        raise RuntimeError("oracle ScanLogo: insufficient logo frames")
    with tempfile.TemporaryDirectory() as td:
        o = os.path.join(td, "oracle.lgd")
        orc.lib.orc_logo_save(lo, o.encode(), b"No Name", 1)                 # the name ScanLogo writes (LogoScan.hpp:1076), serviceid 1
        lgd = open(o, "rb").read()
    out = {"lgd": lgd, "valid_frames": int(nvalid.value), "frames_read": int(nread.value), "threads": T,
           "seconds": {"rectangles_to_host": t1 - t0, "oracle_scanlogo": time.perf_counter() - t1}}
    _ORACLE_LGD[key] = out
    return out


def sharded_scanlogo(ctx, dev, alpha, alphaUV, rank, world, f0, nloc, NT, max_frames=SCANLOGO_MAX_FRAMES, reps=3, verify=True):
    """every rank: the rectangle rows of its frames [f0, f0 + nloc) of the 60-minute stream; amtgpu_scanlogo_sharded through
    torch.distributed (RCCL) -- plain amtgpu_scanlogo at world 1.  lgd_sha256 must not depend on the world size; rank 0 compares the
    file with the CPU oracle's ScanLogo of the whole stream (bytes)."""
    import tempfile
    import torch
    import torch.distributed as dist
    import amt_synth as S
    from amatsukaze_amd import ScanLogo
    from amatsukaze_amd import sharding as SH
    c = S.make_clip_torch(nloc, W, H, 0x5EED0004, alpha, alphaUV, IMGX, IMGY, dev, period=900, fade=12, pitchY=PITCH_Y, pitchUV=PITCH_UV,
                          start=f0, rows=(IMGY, IMGY + LH), flat_every=SCANLOGO_FLAT_EVERY)
    view = _RectView(c, nloc)
    out = os.path.join(tempfile.mkdtemp(), "scan.lgd") if rank == 0 else None
    coll = SH.TorchCollectives() if world > 1 else None

    def run():
        if world > 1:
            ok = SH.scan_logo_sharded(ctx, view, 1, out, IMGX, IMGY, LW, LH, 12, max_frames, coll)
        else:
            ok = ScanLogo(ctx, view, 1, out, IMGX, IMGY, LW, LH, 12, max_frames)
        if not ok or (coll is not None and coll.error is not None):
            raise RuntimeError("sharded ScanLogo failed: " + ctx.lib.amtgpu_last_error(ctx.h).decode(errors="replace"))

    run()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    el = (time.perf_counter() - t0) / reps
    if world > 1:
        tt = torch.tensor([el], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        el = float(tt.item())
    orc = None
    if rank == 0 and verify:
        orc = scanlogo_oracle_lgd(dev, alpha, alphaUV, NT, max_frames, clip=c if world == 1 else None)
    del c
    torch.cuda.empty_cache()
    if rank != 0:
        return None
    lgd = open(out, "rb").read()
    verified = None
    if orc is not None:
        verified = {"frames": NT, "lgd_equals_cpu_oracle": lgd == orc["lgd"], "valid_frames": orc["valid_frames"],
                    "frames_read_before_quota": orc["frames_read"], "quota_hit": orc["valid_frames"] >= max_frames and orc["frames_read"] < NT,
                    "oracle_seconds": orc["seconds"], "oracle_threads": orc["threads"]}
        if not verified["lgd_equals_cpu_oracle"]:
            raise SystemExit(f"sharded ScanLogo verification FAILED at N = {world}: the .lgd of the {NT}-frame stream differs from the CPU oracle's")
    return {"workload": f"ScanLogo over the {NT}-frame stream, frames sharded over {world} GPU(s) by contiguous range, numMaxFrames {max_frames}",
            "value": NT / el, "unit": "frames/sec", "ms_per_scanlogo": el * 1e3, "n_gpus": world, "lgd_sha256": hashlib.sha256(lgd).hexdigest(),
            "verified": verified,
            "note": "lgd_sha256 identical at every N (and to configs.scanlogo_60min.lgd_sha256 of the default line) means the sharded "
                    "ScanLogo writes the single-GPU .lgd byte for byte"}


class _RectView:
    """DeviceClip-shaped description of a rect_rows_clip for the ScanLogo entry points"""

    def __init__(self, c, n):
        self.Y = _DevPtr(c["Y"].data_ptr() - IMGY * PITCH_Y)
        self.U = _DevPtr(c["U"].data_ptr() - (IMGY // 2) * PITCH_UV)
        self.V = _DevPtr(c["V"].data_ptr() - (IMGY // 2) * PITCH_UV)
        self.width, self.height, self.bits, self.num_frames = W, H, 8, n
        self.strideY, self.strideUV, self.pitchY, self.pitchUV = LH * PITCH_Y, (LH // 2) * PITCH_UV, PITCH_Y, PITCH_UV


def config_scanlogo(ctx, dev, logos_np, alpha, alphaUV, args, NT=STRONG_FRAMES, max_frames=None):
    """BASELINE configs[3]'s 'full LogoScan': the exported ScanLogo (LogoScan.hpp:1083-1098, 917-1079) over the 60-minute stream at
    N = 1 -- border test + accumulation over all frames (the first numMaxFrames valid ones), two ReMakeLogo rounds, .lgd written --
    and the .lgd of the WHOLE stream compared with the CPU oracle's ScanLogo (bytes)."""
    import tempfile
    import torch
    import amt_synth as S
    from amatsukaze_amd import ScanLogo
    max_frames = max_frames or args.scanlogo_max_frames
    t0 = time.perf_counter()
    c = S.make_clip_torch(NT, W, H, 0x5EED0004, alpha, alphaUV, IMGX, IMGY, dev, period=900, fade=12, pitchY=PITCH_Y, pitchUV=PITCH_UV,
                          rows=(IMGY, IMGY + LH), flat_every=SCANLOGO_FLAT_EVERY)
    torch.cuda.synchronize()
    gen_s = time.perf_counter() - t0
    view = _RectView(c, NT)
    tmp = tempfile.mkdtemp()
    out = os.path.join(tmp, "scan.lgd")
    state = {"ngather": 0, "nread": 0}

    def cb(progress, nread, total, ngather):
        state["ngather"] = max(state["ngather"], ngather)
        if total == 0:                                                # MakeInitialLogo's progress calls (LogoScan.hpp:904-909): frames read so far
            state["nread"] = max(state["nread"], nread)
        return 1

    def run():
        if not ScanLogo(ctx, view, 1, out, IMGX, IMGY, LW, LH, 12, max_frames, cb):
            raise RuntimeError("ScanLogo failed: " + ctx.lib.amtgpu_last_error(ctx.h).decode(errors="replace"))

    wall, kern = _prof(ctx, run, 3)
    lgd = open(out, "rb").read()
    verified = None
    if not args.no_verify:
        orc = scanlogo_oracle_lgd(dev, alpha, alphaUV, NT, max_frames, clip=c)
        verified = {"frames": NT, "lgd_equals_cpu_oracle": lgd == orc["lgd"], "valid_frames": orc["valid_frames"],
                    "frames_read_before_quota": orc["frames_read"], "quota_hit": orc["valid_frames"] >= max_frames and orc["frames_read"] < NT,
                    "accepted_equals_oracle": state["ngather"] == orc["valid_frames"],
                    "oracle_seconds": orc["seconds"], "oracle_threads": orc["threads"],
                    "how": "the whole stream through the CPU oracle's ScanLogo (quota and accumulations in stream order, the ReMakeLogo rounds' "
                           "per-frame evaluations over the host's cores); .lgd files compared as bytes"}
        if not (verified["lgd_equals_cpu_oracle"] and verified["accepted_equals_oracle"]):
            print(json.dumps({"scanlogo_verified": verified}), file=sys.stderr, flush=True)
            raise SystemExit(f"ScanLogo verification FAILED: the .lgd of the {NT}-frame stream differs from the CPU oracle's")
    del c
    rect_bytes = LW * LH + 2 * (LW // 2) * (LH // 2)
    return {"workload": f"BASELINE configs[3] at N = 1: ScanLogo over the {NT}-frame (60 min) 1440x1080i stream, 256x128 rectangle, thy 12, "
                        f"numMaxFrames {max_frames} (one frame in {SCANLOGO_FLAT_EVERY} has a flat rectangle: {state['ngather']} accepted"
                        + (", the stream-order quota closes the stream early" if state["ngather"] >= max_frames else "") + ")",
            "frames": NT, "accepted_frames": state["ngather"], "value": NT / wall, "unit": "frames/sec", "ms_per_scanlogo": wall * 1e3,
            "kernels_ms_per_call": kern, "algorithmic_bytes": {"border_test_and_accumulate": rect_bytes * NT},
            "lgd_sha256": hashlib.sha256(lgd).hexdigest(), "lgd_bytes": len(lgd), "verified": verified, "clip_generation_s": gen_s,
            "note": "only the rectangle's rows of every frame are resident (30 GB instead of 251 GB): ScanLogo reads nothing else of a frame"}

# --------------------------------------------------------------------------------------------------------------------
# throughput through the drop-in surface itself: the C++ filter classes of include/amt_filters.hpp (the reference's AMTAnalyzeLogo /
# AMTEraseLogo / LogoFrame over the C ABI), frames pulled one GetFrame at a time by a C++ host (tests/cpp/filters_host_test --bench)
# --------------------------------------------------------------------------------------------------------------------
def measure_boundary(ctx, logos, device, frames=6144):
    import tempfile
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-C", cpp, "filters_host_test"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    tmp = tempfile.mkdtemp()
    paths = []
    for i, l in enumerate(logos):
        p = os.path.join(tmp, f"logo{i}.lgd")
        l.save(p, f"bench{i}", 1)
        paths.append(p)
    r = subprocess.run([os.path.join(cpp, "filters_host_test"), "--bench", str(W), str(H), str(frames)] + paths + [str(device)],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("filters_host_test --bench: " + (r.stderr or r.stdout)[-400:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    out["note"] = ("a second process on the same GPU, after the timed region; source frames are handed out by reference (no decoder) and frame "
                   "memory is recycled like AviSynth's frame buffers, so these are the filter layer's own rates: host copies (MakeWritable, "
                   "pinned staging), PCIe, launches.  Round 3's 8-13 k frames/s and its '10 ms tick' were the test source allocating a fresh "
                   "2.3 MB frame per faded picture (profiles/r04_notes.md)")
    return out


def measure_ingest(ctx, logos, alpha, alphaUV, dev):
    """frames that are NOT resident (PCIe inclusive; never `value`): tools/bench_ingest.py"""
    import bench_ingest
    return bench_ingest.measure(ctx, logos, alpha, alphaUV, dev, dict(W=W, H=H, PITCH_Y=PITCH_Y, PITCH_UV=PITCH_UV, IMGX=IMGX, IMGY=IMGY, LH=LH,
                                                                      MASKRATIO=MASKRATIO, ROOT=ROOT))


if __name__ == "__main__":
    main()
