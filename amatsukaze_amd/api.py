"""Python mirror of the reference's interface for the logo / CM / KFM analysis path, on top of the C ABI.

Class names, argument meaning and error behaviour follow the reference (Amatsukaze/LogoScan.hpp):
``LogoFrame(ctx, logofiles, maskratio)`` + ``scanFrames`` / ``selectLogo`` / ``writeResult`` /
``getBestLogo`` / ``getLogoRatio``; ``AMTAnalyzeLogo(clip, logopath, maskratio)``;
``AMTEraseLogo(clip, analyzeclip, logopath, logofpath, mode, maxfade)``; ``ScanLogo(...)``.
A "clip" here is a :class:`DeviceClip`: planar 4:2:0 frames resident in HBM as torch tensors
(torch is plumbing for device memory and streams only).  Failures raise :class:`AmtError` with the
message the C ABI keeps on its context -- there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import binding


class AmtError(RuntimeError):
    pass


def _p(t):
    """device pointer of a torch tensor / host pointer of a numpy array / None"""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return t.ctypes.data_as(C.c_void_p)
    return C.c_void_p(t.data_ptr())


class Context:
    """AMTContext stand-in bound to one GPU (StreamUtils.hpp:343-511)."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        if use_torch_stream:
            # torch BEFORE the library: both link libamdhip64, and the process must end up with one HIP runtime.  With torch's copy
            # loaded first the library binds to it; the other way round torch initialises a second runtime and reports
            # "No HIP GPUs are available".
            import torch
            torch.cuda.init()
        self.lib = binding.load()
        buf = C.create_string_buffer(2048)
        if self.lib.amtgpu_hip_runtimes_loaded(buf, len(buf)) > 1:
            raise AmtError("more than one HIP runtime is mapped into this process (" + ", ".join(buf.value.decode().split()) + "): device "
                           "memory and streams of one are unknown to the other -- load torch (or whichever component brings its own "
                           "libamdhip64) before amatsukaze_amd")
        self.h = self.lib.amtgpu_context_create(device)
        if not self.h:
            raise AmtError(f"amtgpu_context_create({device}) failed: no usable HIP device")
        self.device = device
        if use_torch_stream:
            # Launch on torch's current stream so that kernels are stream-ordered with torch fills / copies / reads of the
            # same tensors.  torch's default stream is the legacy null stream (handle 0), which the ABI spells
            # AMTGPU_STREAM_LEGACY_DEFAULT (NULL would select the context's own non-blocking stream).
            import torch
            hs = int(torch.cuda.current_stream(device).cuda_stream)
            self.lib.amtgpu_context_set_stream(self.h, C.c_void_p(hs if hs else 1))

    def cu_count(self) -> int:
        return self.lib.amtgpu_device_cu_count(self.h)

    def use_cu_range(self, first_cu: int, num_cus: int):
        """Launch this context's kernels on compute units [first_cu, first_cu + num_cus) only (amtgpu_stream_create_cu_range): one
        context per partition lets bandwidth-bound and arithmetic-bound passes run beside each other.  Returns the stream as a
        torch.cuda.ExternalStream so that the caller can order it against other streams (wait_stream / record_event)."""
        import torch
        st = self.lib.amtgpu_stream_create_cu_range(self.h, first_cu, num_cus)
        self.check(st, "stream_create_cu_range")
        self.check(self.lib.amtgpu_context_set_stream(self.h, C.c_void_p(st)))
        self._cu_stream = st
        return torch.cuda.ExternalStream(st, device=self.device)

    def check(self, ok, what=""):
        if not ok:
            raise AmtError((what + ": " if what else "") + self.lib.amtgpu_last_error(self.h).decode(errors="replace"))
        return ok

    def synchronize(self):
        self.check(self.lib.amtgpu_context_synchronize(self.h))

    def profile(self, on: bool = True):
        self.check(self.lib.amtgpu_profile_enable(self.h, 1 if on else 0))

    def profile_report(self):
        """{kernel: (calls, total_ms)} measured with HIP events on the launch stream"""
        buf = C.create_string_buffer(1 << 14)
        n = self.lib.amtgpu_profile_report(self.h, buf, len(buf))
        self.check(n >= 0, "profile_report")
        out = {}
        for line in buf.value.decode().splitlines():
            name, calls, ms = line.split()
            out[name] = (int(calls), float(ms))
        return out

    def close(self):
        if self.h:
            if getattr(self, "_cu_stream", None):
                # (the CU-range stream itself is left to the process: torch may still hold events recorded on its ExternalStream wrapper)
                self.lib.amtgpu_context_synchronize(self.h)
                self.lib.amtgpu_context_set_stream(self.h, None)
                self._cu_stream = None
            self.lib.amtgpu_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class DeviceClip:
    """Frames in HBM: Y (N,H,pitchY), U/V (N,H/2,pitchUV) torch tensors (uint8, or int16/uint16 for >8 bit)."""
    Y: object
    U: object
    V: object
    width: int
    height: int
    bits: int = 8
    fps_num: int = 30000
    fps_den: int = 1001

    @property
    def num_frames(self):
        return int(self.Y.shape[0])

    @property
    def es(self):
        return 1 if self.bits <= 8 else 2

    @property
    def strideY(self):
        return int(self.Y.stride(0)) * self.es

    @property
    def strideUV(self):
        return int(self.U.stride(0)) * self.es

    @property
    def pitchY(self):
        return int(self.Y.stride(1))

    @property
    def pitchUV(self):
        return int(self.U.stride(1))


@dataclass
class DeviceSurfaces:
    """Decoder surfaces in HBM (AmtGpuSurfaces): Y (N,H,pitchY) and, planar, U / V (N,H/2,pitchUV) torch tensors, or interleaved (NV12 /
    P010) U = the UV plane (N,H/2,pitchUV >= width) with V None.  uint8 at 8 bits, int16 / uint16 containers above; msb: the sample sits
    in the high bits of its container (P010 / P012) and is read as container >> (16 - bits)."""
    Y: object
    U: object
    V: object = None
    width: int = 0
    height: int = 0
    bits: int = 8
    interleaved: bool = False
    msb: bool = False

    @property
    def num_frames(self):
        return int(self.Y.shape[0])

    @property
    def es(self):
        return 1 if self.bits <= 8 else 2

    def ref(self):
        """the binding.Surfaces descriptor of these tensors (valid while they live)"""
        for t in (self.Y, self.U, self.V):
            if t is not None and t.element_size() != self.es:
                raise AmtError(f"DeviceSurfaces: {self.es}-byte containers expected at {self.bits} bits, got {t.dtype}")
        return binding.Surfaces(_p(self.Y), _p(self.U), _p(self.V) if self.V is not None else None, int(self.Y.stride(0)) * self.es,
                                int(self.U.stride(0)) * self.es if self.U is not None else 0, int(self.Y.stride(1)),
                                int(self.U.stride(1)) if self.U is not None else 0, self.bits, 1 if self.interleaved else 0, 1 if self.msb else 0, 0)


def extract_rect(ctx: "Context", surfaces: DeviceSurfaces, x, y, w, h):
    """The rectangle (x, y, w, h) of every surface as planar LSB planes (amtgpu_surfaces_extract_rect): (Y [n, h, w], U, V [n, h/2, w/2])
    torch tensors of the surfaces' container type -- what ScanLogoStream.feed_rect and AMTEraseLogo.erase_rect take.  async"""
    import torch
    n = surfaces.num_frames
    dt = surfaces.Y.dtype
    Y = torch.empty((n, h, w), dtype=dt, device=surfaces.Y.device)
    U = torch.empty((n, h // 2, w // 2), dtype=dt, device=surfaces.Y.device)
    V = torch.empty_like(U)
    es = surfaces.es
    d = surfaces.ref()
    ctx.check(ctx.lib.amtgpu_surfaces_extract_rect(ctx.h, C.byref(d), x, y, w, h, n, _p(Y), _p(U), _p(V), int(Y.stride(0)) * es,
                                                   int(U.stride(0)) * es, int(Y.stride(1)), int(U.stride(1))), "extract_rect")
    return Y, U, V


def weave_fields(ctx: "Context", srcY, srcU, srcV, dst: DeviceClip, top_index=None, bottom_index=None, nv12=False, msb=False):
    """AMTSource::MakeFrame -> MergeField (AMTSource.hpp:291-366) on decoded pictures in HBM.

    srcY (P,H,pitch), srcU/srcV (P,H/2,pitch) torch tensors (srcU = the interleaved UV plane and srcV = None for NV12);
    dst frame i = even rows of picture top_index[i], odd rows of picture bottom_index[i] (None = i).
    msb: the pictures are MSB-aligned 16-bit containers (P010 / P012), read as container >> (16 - dst.bits); dst is the usual LSB clip."""
    es = dst.es
    n = dst.num_frames
    ti = (C.c_int * n)(*[int(v) for v in top_index]) if top_index is not None else None
    bi = (C.c_int * n)(*[int(v) for v in bottom_index]) if bottom_index is not None else None
    fn = ctx.lib.amtgpu_weave_fields_batch_msb if msb else ctx.lib.amtgpu_weave_fields_batch
    ctx.check(fn(
        ctx.h, _p(srcY), _p(srcU), _p(srcV) if srcV is not None else None, int(srcY.stride(0)) * es, int(srcU.stride(0)) * es,
        int(srcY.stride(1)), int(srcU.stride(1)), int(srcY.shape[0]), ti, bi, 1 if nv12 else 0, dst.bits, dst.width, dst.height,
        _p(dst.Y), _p(dst.U), _p(dst.V), dst.strideY, dst.strideUV, dst.pitchY, dst.pitchUV, n))


class AmtsFile:
    """The stream-index file AMTSource is built from (amts%d.dat; SaveAMTSource / LoadAMTSource, AMTSource.hpp:835-871)."""

    INFO = ("format", "width", "height", "displayWidth", "displayHeight", "sarWidth", "sarHeight", "frameRateNum", "frameRateDenom",
            "colorPrimaries", "transferCharacteristics", "colorSpace", "progressive", "fixedFrameRate", "audioChannels", "sampleRate",
            "decoderMpeg2", "decoderH264", "decoderHevc")

    def __init__(self, path, ctx: "Context" = None):
        self.ctx = ctx
        self.lib = ctx.lib if ctx else binding.load()
        self.h = self.lib.amtgpu_amts_load(ctx.h if ctx else None, str(path).encode())
        if not self.h:
            raise AmtError(f"cannot read {path}" + (": " + self.lib.amtgpu_last_error(ctx.h).decode(errors="replace") if ctx else ""))
        info = np.zeros(19, np.int32)
        nf, na = C.c_int(), C.c_int()
        self.lib.amtgpu_amts_get_info(self.h, _p(info), C.byref(nf), C.byref(na))
        self.info = dict(zip(self.INFO, map(int, info)))
        self.num_frames, self.num_audio_frames = nf.value, na.value
        cap = 4096
        while True:                                    # (a path is at most 3 UTF-8 bytes per UTF-16 unit: 32 767 units -> < 128 KiB)
            b1, b2 = C.create_string_buffer(cap), C.create_string_buffer(cap)
            if self.lib.amtgpu_amts_get_paths(self.h, b1, cap, b2, cap):
                break
            if cap >= (1 << 20):
                raise AmtError(f"{path}: source / audio path does not fit {cap} bytes")
            cap *= 4
        self.srcpath, self.audiopath = b1.value.decode("utf-8"), b2.value.decode("utf-8")

    def frames(self):
        n = self.num_frames
        out = dict(framePTS=np.zeros(n, np.int64), fileOffset=np.zeros(n, np.int64), keyFrame=np.zeros(n, np.int32),
                   halfDelay=np.zeros(n, np.uint8), cmType=np.zeros(n, np.int32))
        self.lib.amtgpu_amts_get_frames(self.h, _p(out["framePTS"]), _p(out["fileOffset"]), _p(out["keyFrame"]), _p(out["halfDelay"]),
                                        _p(out["cmType"]))
        return out

    def weave_plan(self, picture_pts):
        """(top_index, bottom_index) per frame for decoded pictures with these PTS in output order (AMTSource::OnFrameOutput);
        -1 where the sequence cannot make the frame"""
        pts = np.ascontiguousarray(picture_pts, np.int64)
        top, bot = np.zeros(self.num_frames, np.int32), np.zeros(self.num_frames, np.int32)
        if not self.lib.amtgpu_amts_weave_plan(self.h, _p(pts), len(pts), _p(top), _p(bot)):
            raise AmtError("amtgpu_amts_weave_plan failed")
        return top, bot

    def _fail(self, what):
        return AmtError(what + (": " + self.lib.amtgpu_last_error(self.ctx.h).decode(errors="replace") if self.ctx else ""))

    def audio_info(self):
        """(samples_per_frame, num_samples) of the 16-bit stereo timeline AMTSource presents (MakeVideoInfo): (0, 0) without audio frames"""
        spf, ns = C.c_int(), C.c_int64()
        self.lib.amtgpu_amts_audio_info(self.h, C.byref(spf), C.byref(ns))
        return spf.value, ns.value

    def audio_frames(self):
        n = self.num_audio_frames
        out = dict(frameIndex=np.zeros(n, np.int32), waveOffset=np.zeros(n, np.int64), waveLength=np.zeros(n, np.int32))
        self.lib.amtgpu_amts_get_audio_frames(self.h, _p(out["frameIndex"]), _p(out["waveOffset"]), _p(out["waveLength"]))
        return out

    def read_audio(self, start, count, wavepath=None):
        """AMTSource::GetAudio: `count` sample-frames from `start` on as a (count, 2) int16 array, read from wavepath (None: the file's
        own audiopath); zeros for audio frames without a wave and behind the last audio frame"""
        out = np.zeros((max(0, int(count)), 2), np.int16)
        if not self.lib.amtgpu_amts_read_audio(self.h, str(wavepath).encode() if wavepath is not None else None, int(start), int(count), _p(out)):
            raise self._fail("amtgpu_amts_read_audio failed")
        return out

    def __del__(self):
        try:
            if self.h:
                self.lib.amtgpu_amts_destroy(self.h)
        except Exception:
            pass


class Logo:
    """logo::LogoData + LogoHeader (AMTLogo.hpp:19-280)."""

    def __init__(self, ctx: Context, handle):
        self.ctx, self.h = ctx, handle

    @classmethod
    def load(cls, ctx, path):
        h = ctx.lib.amtgpu_logo_load(ctx.h, str(path).encode())
        ctx.check(h, "LogoData::Load")
        return cls(ctx, h)

    @classmethod
    def from_planes(cls, ctx, planes, w, h, imgw, imgh, imgx, imgy, logUVx=1, logUVy=1):
        planes = np.ascontiguousarray(planes, np.float32)
        hd = ctx.lib.amtgpu_logo_from_planes(ctx.h, w, h, logUVx, logUVy, imgw, imgh, imgx, imgy, _p(planes))
        ctx.check(hd, "logo_from_planes")
        return cls(ctx, hd)

    def save(self, path, name="No Name", service_id=0):
        self.ctx.check(self.ctx.lib.amtgpu_logo_save(self.ctx.h, self.h, str(path).encode(), name.encode(), service_id))

    @property
    def info(self):
        o = np.zeros(8, np.int32)
        self.ctx.lib.amtgpu_logo_get_info(self.h, _p(o))
        return dict(zip(("w", "h", "logUVx", "logUVy", "imgw", "imgh", "imgx", "imgy"), map(int, o)))

    @property
    def planes(self):
        i = self.info
        n = (i["w"] * i["h"] + 2 * (i["w"] >> i["logUVx"]) * (i["h"] >> i["logUVy"])) * 2
        out = np.zeros(n, np.float32)
        self.ctx.lib.amtgpu_logo_get_planes(self.h, _p(out))
        return out

    def mask_tables(self, kind=0, maskratio=0.35):
        i = self.info
        w, h = i["w"], i["h"] if kind == 0 else i["h"] // 2
        mp, cnt, black = C.c_int(), C.c_int(), C.c_float()
        self.ctx.check(self.ctx.lib.amtgpu_logo_mask_tables(self.ctx.h, self.h, kind, maskratio, C.byref(mp), C.byref(cnt), C.byref(black), None, None, None))
        mask = np.zeros(w * h, np.uint8)
        ker = np.zeros(cnt.value * 25, np.float32)
        sc = np.zeros(cnt.value * 64, np.float32)
        self.ctx.check(self.ctx.lib.amtgpu_logo_mask_tables(self.ctx.h, self.h, kind, maskratio, None, None, None, _p(mask), _p(ker), _p(sc)))
        return dict(maskpixels=mp.value, count=cnt.value, blackScore=black.value, mask=mask, kernels=ker, scales=sc)

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.amtgpu_logo_destroy(self.h)
        except Exception:
            pass


class LogoFrame:
    """logo::LogoFrame (LogoScan.hpp:1521-1836)."""

    def __init__(self, ctx: Context, logofiles, maskratio: float):
        self.ctx = ctx
        self.nlogos = len(logofiles)
        if logofiles and isinstance(logofiles[0], Logo):
            arr = (C.c_void_p * self.nlogos)(*[l.h for l in logofiles])
            self._keep = list(logofiles)
            self.h = ctx.lib.amtgpu_logoframe_create_from_logos(ctx.h, arr, self.nlogos, maskratio)
        else:
            arr = (C.c_char_p * self.nlogos)(*[str(p).encode() for p in logofiles])
            self.h = ctx.lib.amtgpu_logoframe_create(ctx.h, arr, self.nlogos, maskratio)
        ctx.check(self.h, "LogoFrame")
        self.num_frames = 0

    def begin(self, width, height, bits, num_frames, fps_num=30000, fps_den=1001):
        self.ctx.check(self.ctx.lib.amtgpu_logoframe_begin(self.h, width, height, bits, num_frames, fps_num, fps_den))
        self.num_frames = num_frames

    def scan_batch(self, Y, bits, first, nframes=None):
        es = 1 if bits <= 8 else 2
        n = int(Y.shape[0]) if nframes is None else nframes
        self.ctx.check(self.ctx.lib.amtgpu_logoframe_scan_batch(self.h, _p(Y), int(Y.stride(0)) * es, int(Y.stride(1)), first, n))

    def scan_surfaces(self, surfaces: "DeviceSurfaces", first):
        """scan_batch on the Y planes of decoder surfaces as they lie (NV12, P010 ...; surfaces.bits must be begin()'s depth).  async"""
        d = surfaces.ref()
        self.ctx.check(self.ctx.lib.amtgpu_logoframe_scan_surfaces(self.h, C.byref(d), first, surfaces.num_frames), "scan_surfaces")

    def scanFrames(self, clip: DeviceClip, batch: int = 4096):
        self.begin(clip.width, clip.height, clip.bits, clip.num_frames, clip.fps_num, clip.fps_den)
        for f0 in range(0, clip.num_frames, batch):
            self.scan_batch(clip.Y[f0:f0 + batch], clip.bits, f0)

    @property
    def evalResults(self):
        out = np.zeros(self.num_frames * self.nlogos * 2, np.float32)
        self.ctx.check(self.ctx.lib.amtgpu_logoframe_get_results(self.h, _p(out)))
        return out.reshape(self.num_frames, self.nlogos, 2)

    def set_results(self, first, evals):
        evals = np.ascontiguousarray(evals, np.float32)
        self.ctx.check(self.ctx.lib.amtgpu_logoframe_set_results(self.h, first, evals.size // (self.nlogos * 2), _p(evals)))

    def selectLogo(self, numCandidates=-1):
        self.ctx.check(self.ctx.lib.amtgpu_logoframe_select_logo(self.h, numCandidates))

    def writeResult(self, outpath, logoIndex=-1):
        self.ctx.check(self.ctx.lib.amtgpu_logoframe_write_result(self.h, str(outpath).encode(), logoIndex))

    def dumpResult(self, basepath):
        """LogoScan.hpp:1632-1643: "<basepath><logo index>", one "%f,%f" line {corr0, corr1} per frame"""
        self.ctx.check(self.ctx.lib.amtgpu_logoframe_dump_result(self.h, str(basepath).encode()))

    def getBestLogo(self):
        return self.ctx.lib.amtgpu_logoframe_best_logo(self.h)

    def getLogoRatio(self):
        return self.ctx.lib.amtgpu_logoframe_logo_ratio(self.h)

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.amtgpu_logoframe_destroy(self.h)
        except Exception:
            pass


def logoframe_decide_host(evals, fps_num=30000, fps_den=1001, numCandidates=-1, logoIndex=-1):
    """LogoFrame::selectLogo + the text of writeResult (LogoScan.hpp:1647-1827) from scan records [frames][logos][2] alone -- host only,
    no device: (bestLogo, logoRatio, text bytes).  What every rank computes after the all-gather of the records."""
    lib = binding.load()
    ev = np.ascontiguousarray(evals, np.float32)
    n, nl = int(ev.shape[0]), int(ev.shape[1])
    best, ratio, tl = C.c_int(-1), C.c_float(0.0), C.c_int(0)
    args = (_p(ev), n, nl, numCandidates, logoIndex, fps_num, fps_den, C.byref(best), C.byref(ratio))
    if lib.amtgpu_logoframe_decide_host(*args, None, 0, C.byref(tl)) != 1:
        raise AmtError("amtgpu_logoframe_decide_host: bad arguments")
    buf = C.create_string_buffer(max(1, tl.value))
    if lib.amtgpu_logoframe_decide_host(*args, buf, tl.value, C.byref(tl)) != 1:
        raise AmtError("amtgpu_logoframe_decide_host failed")
    return best.value, ratio.value, buf.raw[:tl.value]


class AMTAnalyzeLogo:
    """logo::AMTAnalyzeLogo (LogoScan.hpp:1106-1236); GetFrames returns 33 floats per source frame."""

    MODES = {"exact": 0, "linear": 1, "linear_unguarded": 2, "monitored": 3}

    def __init__(self, ctx: Context, logo, maskratio: float = 0.35, mode: str = "exact", tolerance: float = 1e-4, sentinels: int = 16):
        """mode "exact": records bit-identical to the reference's; "linear": all fades from one evaluation of the source and one
        of the background window per mask pixel (scores within `error_bound` of the reference's, decisions guarded by exact
        re-evaluation -- include/amt_gpu.h AMTGPU_ANALYZE_LINEAR_GUARDED); "monitored": "linear", and `sentinels` frames of every batch
        are evaluated exactly as well and compared on the device: a score off by more than `tolerance` re-evaluates the batch exactly and
        keeps the analyzer exact from then on (AMTGPU_ANALYZE_LINEAR_MONITORED)."""
        self.ctx = ctx
        if isinstance(logo, Logo):
            self._keep = logo
            self.h = ctx.lib.amtgpu_analyze_create_from_logo(ctx.h, logo.h, maskratio)
        else:
            self.h = ctx.lib.amtgpu_analyze_create(ctx.h, str(logo).encode(), maskratio)
        ctx.check(self.h, "AMTAnalyzeLogo")
        if mode == "monitored" or (tolerance, sentinels) != (1e-4, 16):
            self.set_monitor(tolerance, sentinels)
        self.set_mode(mode)

    def set_mode(self, mode: str):
        """switches the evaluation mode; "monitored" (also when already set) re-arms the monitor"""
        self.ctx.check(self.ctx.lib.amtgpu_analyze_set_mode(self.h, self.MODES[mode]))

    def set_monitor(self, tolerance: float = 1e-4, sentinels: int = 16):
        """the monitored mode's tolerance on |linear - exact| and sentinel frames per batch, from the next batch on"""
        self.ctx.check(self.ctx.lib.amtgpu_analyze_set_monitor(self.h, float(tolerance), int(sentinels)))

    def monitor_stats(self):
        """since the monitor was armed: {"max_abs": largest |linear - exact| compared, "frames_checked", "downgraded": bool} (synchronises)"""
        m, n, d = C.c_float(), C.c_int64(), C.c_int()
        self.ctx.check(self.ctx.lib.amtgpu_analyze_monitor_stats(self.h, C.byref(m), C.byref(n), C.byref(d)))
        return {"max_abs": m.value, "frames_checked": n.value, "downgraded": bool(d.value)}

    def last_refined(self):
        return self.ctx.lib.amtgpu_analyze_last_refined(self.h)

    def set_fixup_queue(self, entries):
        """pairs a wave of the linear kernel can list for the exact bin check (a tuning knob; results do not depend on it)"""
        self.ctx.check(self.ctx.lib.amtgpu_analyze_set_fixup_queue(self.h, int(entries)))

    def error_bound(self, group=0, bits=8):
        return self.ctx.lib.amtgpu_analyze_error_bound(self.h, group, bits)

    def analyze_device(self, Y, bits, out):
        es = 1 if bits <= 8 else 2
        self.ctx.check(self.ctx.lib.amtgpu_analyze_batch(self.h, _p(Y), int(Y.stride(0)) * es, int(Y.stride(1)), bits, int(Y.shape[0]), _p(out)))

    def analyze_surfaces(self, surfaces: "DeviceSurfaces", out=None):
        """analyze_device on the Y planes of decoder surfaces as they lie (NV12, P010 ...): the device tensor [n, 33] of records.  async"""
        import torch
        if out is None:
            out = torch.empty((surfaces.num_frames, 33), dtype=torch.float32, device=surfaces.Y.device)
        d = surfaces.ref()
        self.ctx.check(self.ctx.lib.amtgpu_analyze_surfaces(self.h, C.byref(d), surfaces.num_frames, _p(out)), "analyze_surfaces")
        return out

    def analyze(self, clip: DeviceClip):
        out = np.zeros((clip.num_frames, 33), np.float32)
        self.ctx.check(self.ctx.lib.amtgpu_analyze_batch_host(self.h, _p(clip.Y), clip.strideY, clip.pitchY, clip.bits, clip.num_frames, _p(out)))
        return out

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.amtgpu_analyze_destroy(self.h)
        except Exception:
            pass


class AMTEraseLogo:
    """logo::AMTEraseLogo (LogoScan.hpp:1238-1519), mode 0."""

    def __init__(self, ctx: Context, logo, logof="", mode: int = 0, maxfade: int = 16):
        self.ctx = ctx
        if isinstance(logo, Logo):
            self._keep = logo
            self.h = ctx.lib.amtgpu_erase_create_from_logo(ctx.h, logo.h, (logof or "").encode(), mode, maxfade)
        else:
            self.h = ctx.lib.amtgpu_erase_create(ctx.h, str(logo).encode(), str(logof or "").encode(), mode, maxfade)
        ctx.check(self.h, "AMTEraseLogo")

    def calc_fades(self, analysis, num_frames, first=0, nframes=None):
        analysis = np.ascontiguousarray(analysis, np.float32)
        n = num_frames - first if nframes is None else nframes
        out = np.zeros((n, 2), np.float32)
        self.ctx.check(self.ctx.lib.amtgpu_erase_calc_fades(self.h, _p(analysis), num_frames, first, n, _p(out)))
        return out

    def calc_fades_device(self, d_analysis, num_frames, first=0, nframes=None, analysis_first=0, out=None):
        """CalcFade / CalcFade2 on the device: d_analysis = torch float32 [count, 33] records of source frames
        [analysis_first, analysis_first + count) still in HBM; returns a torch float32 [nframes, 2] tensor (async)."""
        import torch
        n = num_frames - first if nframes is None else nframes
        if out is None:
            out = torch.empty((n, 2), dtype=torch.float32, device=d_analysis.device)
        self.ctx.check(self.ctx.lib.amtgpu_erase_calc_fades_device(self.h, _p(d_analysis), analysis_first, int(d_analysis.shape[0]), num_frames,
                                                                   first, n, _p(out)))
        return out

    def erase_device_fades(self, clip: DeviceClip, d_fades, dst: "DeviceClip | None" = None):
        """Delogo with fades that are already on the device (calc_fades_device's output).  async
        dst: a batch of the same geometry that already holds a copy of clip's frames -- the writable copy AMTEraseLogo::GetFrameT takes
        (env->MakeWritable, LogoScan.hpp:1346-1347): Delogo reads clip and writes dst's rectangle, clip stays intact.  None: in place."""
        if dst is None:
            self.ctx.check(self.ctx.lib.amtgpu_erase_batch_dfades(self.h, _p(clip.Y), _p(clip.U), _p(clip.V), clip.strideY, clip.strideUV,
                                                                  clip.pitchY, clip.pitchUV, clip.bits, clip.num_frames, _p(d_fades)))
            return
        same = ("strideY", "strideUV", "pitchY", "pitchUV", "bits", "num_frames")
        if any(getattr(clip, k) != getattr(dst, k) for k in same):
            raise ValueError("erase_device_fades: source and destination batches differ in geometry")
        self.ctx.check(self.ctx.lib.amtgpu_erase_batch_dfades_to(self.h, _p(clip.Y), _p(clip.U), _p(clip.V), _p(dst.Y), _p(dst.U), _p(dst.V),
                                                                 clip.strideY, clip.strideUV, clip.pitchY, clip.pitchUV, clip.bits,
                                                                 clip.num_frames, _p(d_fades)))

    def erase_surfaces(self, surfaces: "DeviceSurfaces", fades=None, d_fades=None, dst: "DeviceSurfaces | None" = None):
        """Delogo on decoder surfaces where they lie (NV12, P010 / P012, planar MSB): the logo rectangle of `surfaces` is REWRITTEN in place.
        Exactly one of fades (host, [n, 2]) / d_fades (device, e.g. calc_fades_device's output).  dst (with d_fades only): surfaces of the
        same layout that already hold a copy of the pictures; Delogo then reads `surfaces` and writes dst's rectangle.  async"""
        if (fades is None) == (d_fades is None):
            raise ValueError("erase_surfaces: exactly one of fades / d_fades")
        if dst is not None and d_fades is None:
            raise ValueError("erase_surfaces: dst needs d_fades")
        n = surfaces.num_frames
        d = surfaces.ref()
        if d_fades is None:
            fades = np.ascontiguousarray(fades, np.float32)
            if fades.size != 2 * n:
                raise ValueError("erase_surfaces: fades must hold two floats per frame")
            self.ctx.check(self.ctx.lib.amtgpu_erase_surfaces(self.h, C.byref(d), n, _p(fades)), "erase_surfaces")
        elif dst is None:
            self.ctx.check(self.ctx.lib.amtgpu_erase_surfaces_dfades(self.h, C.byref(d), n, _p(d_fades)), "erase_surfaces")
        else:
            if dst.num_frames != n:
                raise ValueError("erase_surfaces: source and destination batches differ in frame count")
            dd = dst.ref()
            self.ctx.check(self.ctx.lib.amtgpu_erase_surfaces_dfades_to(self.h, C.byref(d), C.byref(dd), n, _p(d_fades)), "erase_surfaces")

    def erase(self, clip: DeviceClip, fades):
        fades = np.ascontiguousarray(fades, np.float32)
        self.ctx.check(self.ctx.lib.amtgpu_erase_batch(self.h, _p(clip.Y), _p(clip.U), _p(clip.V), clip.strideY, clip.strideUV,
                                                       clip.pitchY, clip.pitchUV, clip.bits, clip.num_frames, _p(fades)))

    @property
    def rect(self):
        """(imgx, imgy, w, h, fade0_is_identity): the rectangle Delogo rewrites"""
        out = (C.c_int * 5)()
        self.ctx.check(self.ctx.lib.amtgpu_erase_get_rect(self.h, out), "erase_get_rect")
        return tuple(out)

    def erase_rect(self, Y, U, V, bits, fades):
        """Delogo on device planes that hold only the logo rectangle: Y [n, h, w], U / V [n, h/2, w/2] (any row pitch)"""
        fades = np.ascontiguousarray(fades, np.float32)
        es = 1 if bits <= 8 else 2
        self.ctx.check(self.ctx.lib.amtgpu_erase_rect_batch(self.h, _p(Y), _p(U), _p(V), int(Y.stride(0)) * es, int(U.stride(0)) * es,
                                                            int(Y.stride(1)), int(U.stride(1)), bits, int(Y.shape[0]), _p(fades)))

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.amtgpu_erase_destroy(self.h)
        except Exception:
            pass


class LogoScan:
    """logo::LogoScan (LogoScan.hpp:398-660) with exact integer accumulators."""

    def __init__(self, ctx: Context, w, h, thy, logUVx=1, logUVy=1):
        self.ctx, self.w, self.hh = ctx, w, h
        self.h = ctx.lib.amtgpu_logoscan_create(ctx.h, w, h, logUVx, logUVy, thy)
        ctx.check(self.h, "LogoScan")

    def add_batch(self, clip: DeviceClip, imgx, imgy, max_valid=1 << 30, use_mask=None):
        valid = np.zeros(clip.num_frames, np.uint8)
        n = C.c_int()
        um = None if use_mask is None else np.ascontiguousarray(use_mask, np.uint8)
        self.ctx.check(self.ctx.lib.amtgpu_logoscan_add_batch(self.h, _p(clip.Y), _p(clip.U), _p(clip.V), clip.strideY, clip.strideUV,
                                                              clip.pitchY, clip.pitchUV, clip.bits, imgx, imgy, clip.num_frames,
                                                              max_valid, _p(um), _p(valid), C.byref(n)))
        return valid, n.value

    @property
    def nframes(self):
        return self.ctx.lib.amtgpu_logoscan_nframes(self.h)

    def sums(self):
        npx = self.w * self.hh + 2 * (self.w // 2) * (self.hh // 2)
        s = np.zeros(npx * 3, np.int64)
        p = np.zeros(6, np.int64)
        self.ctx.check(self.ctx.lib.amtgpu_logoscan_get_sums(self.h, _p(s), _p(p)))
        return s, p

    def set_sums(self, s, p, nframes):
        s = np.ascontiguousarray(s, np.int64)
        p = np.ascontiguousarray(p, np.int64)
        self.ctx.check(self.ctx.lib.amtgpu_logoscan_set_sums(self.h, _p(s), _p(p), nframes))

    def get_logo(self, maxv, clean, imgw, imgh, imgx, imgy):
        h = self.ctx.lib.amtgpu_logoscan_get_logo(self.h, maxv, 1 if clean else 0, imgw, imgh, imgx, imgy)
        self.ctx.check(h, "LogoScan::GetLogo")
        return Logo(self.ctx, h)

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.amtgpu_logoscan_destroy(self.h)
        except Exception:
            pass


def ScanLogo(ctx: Context, clip: DeviceClip, serviceid, dstpath, imgx, imgy, w, h, thy, numMaxFrames, cb=None):
    """The exported ScanLogo (LogoScan.hpp:1083-1098) over a device clip; returns True/False like it.  The clip's depth is clip.bits
    (8, or 9..12 in 16-bit containers); thy is in container units of that depth."""
    cbf = binding.CB(cb) if cb else binding.CB(lambda p, a, b, c: 1)
    planes = (ctx.h, _p(clip.Y), _p(clip.U), _p(clip.V), clip.strideY, clip.strideUV, clip.pitchY, clip.pitchUV, clip.width, clip.height)
    rest = (clip.num_frames, serviceid, str(dstpath).encode(), imgx, imgy, w, h, thy, numMaxFrames, cbf)
    if clip.bits == 8:
        return bool(ctx.lib.amtgpu_scanlogo(*planes, *rest))
    return bool(ctx.lib.amtgpu_scanlogo_bits(*planes, clip.bits, *rest))


def ScanLogoFile(ctx: Context, srcpath, serviceid, workfile, dstpath, imgx, imgy, w, h, thy, numMaxFrames, cb=None):
    """ScanLogo with the reference's own argument list (LogoScan.hpp:1083-1098) over a raw clip file ('AMTR': 8-bit, 'AMTH': 9..12-bit);
    True/False like it."""
    cbf = binding.CB(cb) if cb else binding.CB(lambda p, a, b, c: 1)
    return bool(ctx.lib.amtgpu_scanlogo_file(ctx.h, str(srcpath).encode(), serviceid, str(workfile).encode(), str(dstpath).encode(), imgx, imgy,
                                             w, h, thy, numMaxFrames, cbf))


@dataclass
class LogoCandidate:
    """AmtGpuLogoRect: a rectangle for ScanLogo (imgx, imgy, w, h: even, inside the frame) and how strongly it was found"""
    imgx: int
    imgy: int
    w: int
    h: int
    score: float
    coherence: float
    edge_pixels: int

    @classmethod
    def _of(cls, r):
        return cls(r.imgx, r.imgy, r.w, r.h, r.score, r.coherence, r.edge_pixels)


def logo_find_params(**params):
    """AmtGpuLogoFindParams: the library's defaults with the given fields replaced (min_coherence, min_edge, join, margin, min_w,
    min_h, max_w_frac, max_h_frac)"""
    p = binding.LogoFindParams()
    binding.load().amtgpu_logofind_default_params(C.byref(p))
    for k, v in params.items():
        if k not in dict(binding.LogoFindParams._fields_):
            raise TypeError(f"unknown logo-finder parameter {k!r}")
        setattr(p, k, v)
    return p


def logo_candidates_host(sums, width, height, bits, nframes, cap=64, **params):
    """amtgpu_logofind_candidates_host: ranked candidates from sums in host memory (2*W*H int64: S1 then SM); no device.
    Returns (candidates, total) or raises ValueError when the library refuses the arguments."""
    s = np.ascontiguousarray(sums, np.int64)
    out = (binding.LogoRect * max(1, cap))()
    n = C.c_int()
    p = logo_find_params(**params)
    if not binding.load().amtgpu_logofind_candidates_host(_p(s), width, height, bits, nframes, C.byref(p), out, cap, C.byref(n)):
        raise ValueError("amtgpu_logofind_candidates_host refused its arguments")
    return [LogoCandidate._of(out[i]) for i in range(min(cap, n.value))], n.value


class LogoFinder:
    """Automatic logo detection (self-specified): edge-persistence sums over the Y planes of every frame
    offered, then ranked candidate rectangles for ScanLogo."""

    def __init__(self, ctx: Context, width, height, bits=8):
        self.ctx, self.width, self.height, self.bits = ctx, width, height, bits
        self.h = ctx.lib.amtgpu_logofind_create(ctx.h, width, height, bits)
        ctx.check(self.h, "LogoFinder")

    def add_device(self, Y, nframes=None):
        """Y: torch tensor (N, H, pitch) of Y planes in HBM (uint8, or int16 / uint16 above 8 bits).  async"""
        es = 1 if self.bits <= 8 else 2
        n = int(Y.shape[0]) if nframes is None else nframes
        self.ctx.check(self.ctx.lib.amtgpu_logofind_add_batch(self.h, _p(Y), int(Y.stride(0)) * es, int(Y.stride(1)), n))

    def add(self, clip: DeviceClip):
        self.add_device(clip.Y)

    def add_surfaces(self, surfaces: DeviceSurfaces):
        """the Y planes of decoder surfaces (NV12, P010, ...; MSB-aligned ones are summed as container >> (16 - bits)).  async"""
        d = surfaces.ref()
        self.ctx.check(self.ctx.lib.amtgpu_logofind_add_surfaces(self.h, C.byref(d), surfaces.num_frames))

    @property
    def nframes(self):
        return int(self.ctx.lib.amtgpu_logofind_nframes(self.h))

    def sums(self):
        """(S1, SM): int64 arrays of shape (H, W)"""
        s = np.zeros(2 * self.width * self.height, np.int64)
        self.ctx.check(self.ctx.lib.amtgpu_logofind_get_sums(self.h, _p(s)))
        s = s.reshape(2, self.height, self.width)
        return s[0], s[1]

    def set_sums(self, S1, SM, nframes):
        s = np.ascontiguousarray(np.concatenate([np.ravel(S1), np.ravel(SM)]), np.int64)
        if s.size != 2 * self.width * self.height:
            raise ValueError("set_sums: sums of another frame size")
        self.ctx.check(self.ctx.lib.amtgpu_logofind_set_sums(self.h, _p(s), nframes))

    def allreduce(self, coll):
        """frame-sharded detection: every rank's sums (and frame count) summed on every rank (sharding.TorchCollectives)"""
        self.ctx.check(self.ctx.lib.amtgpu_logofind_allreduce(self.h, coll.ref()))

    def candidates(self, cap=64, **params):
        """ranked LogoCandidate list (at most cap); parameters as in logo_find_params"""
        out = (binding.LogoRect * max(1, cap))()
        n = C.c_int()
        p = logo_find_params(**params)
        self.ctx.check(self.ctx.lib.amtgpu_logofind_candidates(self.h, C.byref(p), out, cap, C.byref(n)))
        return [LogoCandidate._of(out[i]) for i in range(min(cap, n.value))]

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.amtgpu_logofind_destroy(self.h)
        except Exception:
            pass


def ScanLogoAuto(ctx: Context, clip: DeviceClip, serviceid, dstpath, thy, numMaxFrames, cb=None, **params):
    """ScanLogo without a rectangle: detection over the whole clip, then ScanLogo on the best candidate.  Returns (ok, LogoCandidate or
    None); with no candidate ok is False and the context's message is "no logo found".  Detection and scan run at clip.bits."""
    cbf = binding.CB(cb) if cb else binding.CB(lambda p, a, b, c: 1)
    found = binding.LogoRect()
    p = logo_find_params(**params)
    planes = (ctx.h, _p(clip.Y), _p(clip.U), _p(clip.V), clip.strideY, clip.strideUV, clip.pitchY, clip.pitchUV, clip.width, clip.height)
    rest = (clip.num_frames, serviceid, str(dstpath).encode() if dstpath else None, thy, numMaxFrames, cbf, C.byref(p), C.byref(found))
    if clip.bits == 8:
        ok = ctx.lib.amtgpu_scanlogo_auto(*planes, *rest)
    else:
        ok = ctx.lib.amtgpu_scanlogo_auto_bits(*planes, clip.bits, *rest)
    return bool(ok), (LogoCandidate._of(found) if found.w > 0 else None)


def ScanLogoFileAuto(ctx: Context, srcpath, serviceid, workfile, dstpath, thy, numMaxFrames, cb=None, **params):
    """ScanLogoFile without a rectangle (the raw 'AMTR' / 'AMTH' clip is read twice); returns (ok, LogoCandidate or None)"""
    cbf = binding.CB(cb) if cb else binding.CB(lambda p, a, b, c: 1)
    found = binding.LogoRect()
    p = logo_find_params(**params)
    ok = ctx.lib.amtgpu_scanlogo_file_auto(ctx.h, str(srcpath).encode(), serviceid, str(workfile).encode(), str(dstpath).encode(), thy,
                                           numMaxFrames, cbf, C.byref(p), C.byref(found))
    return bool(ok), (LogoCandidate._of(found) if found.w > 0 else None)


class ScanLogoStream:
    """ScanLogo as a session fed with frame batches (amtgpu_scanlogo_stream_*): for a clip that is decoded as it goes and never
    resident.  feed / feed_rect return (frames kept so far, done); finish writes the .lgd -- byte-identical to ScanLogo over the same
    frames -- and returns True / False like ScanLogo (the message stays on the context).  A batch may be overwritten by work on the
    context's stream as soon as its feed has returned.  bits: the depth of every frame fed (8, or 9..12 in 16-bit containers)."""

    def __init__(self, ctx: Context, imgw, imgh, imgx, imgy, w, h, thy, numMaxFrames, bits=8):
        self.ctx, self.bits = ctx, bits
        if bits == 8:
            self.h = ctx.lib.amtgpu_scanlogo_stream_create(ctx.h, imgw, imgh, imgx, imgy, w, h, thy, numMaxFrames)
        else:
            self.h = ctx.lib.amtgpu_scanlogo_stream_create_bits(ctx.h, imgw, imgh, bits, imgx, imgy, w, h, thy, numMaxFrames)
        ctx.check(self.h, "ScanLogoStream")

    def _fed(self, fn, Y, U, V, strideY, strideUV, pitchY, pitchUV, n):
        nkept, done = C.c_int(), C.c_int()
        self.ctx.check(fn(self.h, _p(Y), _p(U), _p(V), strideY, strideUV, pitchY, pitchUV, n, C.byref(nkept), C.byref(done)), "ScanLogoStream")
        return nkept.value, bool(done.value)

    def feed(self, clip: DeviceClip):
        """the next frames of the stream, full frames of the session's depth"""
        if clip.bits != self.bits:
            raise AmtError(f"ScanLogoStream: a {clip.bits}-bit clip fed to a {self.bits}-bit session")
        return self._fed(self.ctx.lib.amtgpu_scanlogo_stream_feed, clip.Y, clip.U, clip.V, clip.strideY, clip.strideUV, clip.pitchY,
                         clip.pitchUV, clip.num_frames)

    def feed_rect(self, Y, U, V):
        """the same on device planes that hold only the rectangle: Y [n, h, w], U / V [n, h/2, w/2] (any row pitch); uint8, or int16 /
        uint16 when the session is deeper than 8 bits"""
        es = 1 if self.bits <= 8 else 2
        for t in (Y, U, V):
            if t.element_size() != es:
                raise AmtError(f"ScanLogoStream: {es}-byte samples expected for a {self.bits}-bit session, got {t.dtype}")
        return self._fed(self.ctx.lib.amtgpu_scanlogo_stream_feed_rect, Y, U, V, int(Y.stride(0)) * es, int(U.stride(0)) * es, int(Y.stride(1)),
                         int(U.stride(1)), int(Y.shape[0]))

    def feed_surfaces(self, surfaces: DeviceSurfaces):
        """the same on decoder surfaces (NV12, P010, planar MSB ...) of the session's depth: only the rectangle is read"""
        d = surfaces.ref()
        nkept, done = C.c_int(), C.c_int()
        self.ctx.check(self.ctx.lib.amtgpu_scanlogo_stream_feed_surfaces(self.h, C.byref(d), surfaces.num_frames, C.byref(nkept), C.byref(done)),
                       "ScanLogoStream")
        return nkept.value, bool(done.value)

    def status(self):
        """{"nread": frames consumed up to and including the one that closed the stream, "nkept", "done"}"""
        nread, nkept, done = C.c_int64(), C.c_int(), C.c_int()
        self.ctx.check(self.ctx.lib.amtgpu_scanlogo_stream_status(self.h, C.byref(nread), C.byref(nkept), C.byref(done)))
        return {"nread": nread.value, "nkept": nkept.value, "done": bool(done.value)}

    def finish(self, serviceid, dstpath, cb=None):
        cbf = binding.CB(cb) if cb else binding.CB(lambda p, a, b, c: 1)
        return bool(self.ctx.lib.amtgpu_scanlogo_stream_finish(self.h, serviceid, str(dstpath).encode(), cbf))

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.amtgpu_scanlogo_stream_destroy(self.h)
        except Exception:
            pass


def ScanLogoAutoStream(ctx: Context, batches, width, height, serviceid, dstpath, thy, numMaxFrames, cb=None, bits=8, **params):
    """ScanLogoAuto over a clip that is streamed, not resident: `batches` is a callable that returns a fresh iterator of DeviceClip
    or DeviceSurfaces batches (`bits` deep, in stream order; each batch is taken as what it is).  Pass 1 feeds every batch to a LogoFinder; pass 2 feeds a ScanLogoStream on the best candidate and
    stops iterating once its quota is full.  Returns the LogoCandidate; raises AmtError ("no logo found", or ScanLogo's message)."""
    finder = LogoFinder(ctx, width, height, bits)
    for clip in batches():
        if isinstance(clip, DeviceSurfaces):
            finder.add_surfaces(clip)
        else:
            finder.add(clip)
    cands = finder.candidates(1, **params)
    if not cands:
        raise AmtError("no logo found")
    r = cands[0]
    stream = ScanLogoStream(ctx, width, height, r.imgx, r.imgy, r.w, r.h, thy, numMaxFrames, bits=bits)
    for clip in batches():
        if (stream.feed_surfaces(clip) if isinstance(clip, DeviceSurfaces) else stream.feed(clip))[1]:
            break
    ctx.check(stream.finish(serviceid, dstpath, cb), "ScanLogoStream")
    return r


class FrameStats:
    """Self-specified whole-frame field-difference / combing metrics."""

    def __init__(self, ctx: Context, width, height, bits=8):
        self.ctx, self.width, self.height, self.bits = ctx, width, height, bits
        self.h = ctx.lib.amtgpu_framestats_create(ctx.h, width, height, bits)
        ctx.check(self.h, "FrameStats")

    def run_device(self, Y, out, prevY=None):
        es = 1 if self.bits <= 8 else 2
        self.ctx.check(self.ctx.lib.amtgpu_framestats_batch(self.h, _p(Y), int(Y.stride(0)) * es, int(Y.stride(1)), _p(prevY), int(Y.shape[0]), _p(out)))

    def run(self, clip: DeviceClip):
        import torch
        out = torch.zeros((clip.num_frames, 8), dtype=torch.int64, device=clip.Y.device)
        self.run_device(clip.Y, out)
        self.ctx.synchronize()
        return out.cpu().numpy().astype(np.uint64)

    def run_device_surfaces(self, surfaces: DeviceSurfaces, out, prev: DeviceSurfaces = None):
        """the metrics of the Y planes of decoder surfaces (NV12, P010, ...; MSB-aligned ones are read as container >> (16 - bits) inside
        the kernel); prev: the ONE picture before the batch, of the same depth, alignment and pitch; out: (N, 8) int64 in HBM.  async"""
        d = surfaces.ref()
        dp = prev.ref() if prev is not None else None
        self.ctx.check(self.ctx.lib.amtgpu_framestats_surfaces(self.h, C.byref(d), C.byref(dp) if dp is not None else None, surfaces.num_frames,
                                                               _p(out)))

    def run_surfaces(self, surfaces: DeviceSurfaces, prev: DeviceSurfaces = None):
        import torch
        out = torch.zeros((surfaces.num_frames, 8), dtype=torch.int64, device=surfaces.Y.device)
        self.run_device_surfaces(surfaces, out, prev)
        self.ctx.synchronize()
        return out.cpu().numpy().astype(np.uint64)

    def scene_changes(self, metrics):
        m = np.ascontiguousarray(metrics, np.uint64)
        n = m.shape[0]
        out = np.zeros(max(1, n), np.int32)
        k = C.c_int()
        self.ctx.lib.amtgpu_cm_scene_changes(_p(m), n, self.width, self.height, _p(out), n, C.byref(k))
        return out[:k.value].copy()

    def cadence(self, metrics):
        m = np.ascontiguousarray(metrics, np.uint64)
        n = m.shape[0]
        cad = np.zeros(n, np.uint8)
        ph = np.zeros(n, np.uint8)
        self.ctx.lib.amtgpu_kfm_cadence(_p(m), n, self.width, self.height, _p(cad), _p(ph))
        return cad, ph

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.amtgpu_framestats_destroy(self.h)
        except Exception:
            pass


class AudioLevels:
    """Per-video-frame audio levels: (N, 4) uint64 records {PEAK, SUMABS, SUMSQ, COUNT} of interleaved int16 PCM.
    Video frame n owns sample-frames [frame_start(n), frame_start(n + 1)) below num_samples."""

    PEAK, SUMABS, SUMSQ, COUNT = 0, 1, 2, 3

    def __init__(self, ctx: Context, sample_rate, channels, fps_num, fps_den, num_samples):
        self.ctx, self.sample_rate, self.channels, self.fps_num, self.fps_den = ctx, sample_rate, channels, fps_num, fps_den
        self.num_samples = int(num_samples)
        self.h = ctx.lib.amtgpu_audiolevels_create(ctx.h, sample_rate, channels, fps_num, fps_den, self.num_samples)
        ctx.check(self.h, "AudioLevels")

    def frame_start(self, n):
        return int(self.ctx.lib.amtgpu_audiolevels_frame_start(self.h, int(n)))

    def num_frames(self):
        """video frames that own at least one sample-frame"""
        n = self.num_samples * self.fps_num // (self.sample_rate * self.fps_den)
        while self.frame_start(n) < self.num_samples:
            n += 1
        while n > 0 and self.frame_start(n - 1) >= self.num_samples:
            n -= 1
        return n

    def run_device(self, pcm, pcm_first, first_frame, nframes, out=None):
        """pcm: torch int16 tensor in HBM whose elements are sample-frames pcm_first .. of the timeline, interleaved (any shape; it must be
        contiguous); out: (nframes, 4) int64 in HBM, made when None.  async"""
        import torch
        if pcm.dtype != torch.int16 or not pcm.is_contiguous():
            raise AmtError("AudioLevels: pcm must be a contiguous int16 tensor")
        if out is None:
            out = torch.zeros((nframes, 4), dtype=torch.int64, device=pcm.device)
        self.ctx.check(self.ctx.lib.amtgpu_audiolevels_batch(self.h, _p(pcm), int(pcm_first), pcm.numel() // self.channels, int(first_frame),
                                                            int(nframes), _p(out)), "AudioLevels")
        return out

    def run(self, pcm_numpy, first_frame=0, nframes=None):
        """pcm_numpy: the whole timeline from sample-frame 0 on, int16, (samples, channels) or flat interleaved"""
        import torch
        host = np.ascontiguousarray(pcm_numpy, np.int16).reshape(-1)
        pcm = torch.from_numpy(host if host.flags.writeable else host.copy()).cuda(self.ctx.device)
        if nframes is None:
            nframes = self.num_frames() - first_frame
        out = self.run_device(pcm, 0, first_frame, nframes)
        self.ctx.synchronize()
        return out.cpu().numpy().astype(np.uint64)

    def run_amts(self, amts: AmtsFile, wavepath=None, first_frame=0, nframes=None):
        """the records of the audio an amts file describes (AmtsFile.read_audio's samples), read, uploaded and reduced in chunks"""
        if nframes is None:
            nframes = self.num_frames() - first_frame
        out = np.zeros((nframes, 4), np.uint64)
        self.ctx.check(self.ctx.lib.amtgpu_audiolevels_amts(self.h, amts.h, str(wavepath).encode() if wavepath is not None else None,
                                                           int(first_frame), int(nframes), _p(out)), "AudioLevels")
        return out

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.amtgpu_audiolevels_destroy(self.h)
        except Exception:
            pass


def mute_sections(levels, mute_level=50, min_frames=10):
    """[(start, end)] inclusive runs of at least min_frames video frames whose PEAK is at most mute_level (or that own no samples)"""
    lv = np.ascontiguousarray(levels, np.uint64).reshape(-1, 4)
    n = lv.shape[0]
    lib = binding.load()
    cap = n // max(1, int(min_frames)) + 1
    st, en = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    k = C.c_int()
    if not lib.amtgpu_cm_mute_sections(_p(lv), n, int(mute_level), int(min_frames), _p(st), _p(en), cap, C.byref(k)):
        raise AmtError("amtgpu_cm_mute_sections failed (min_frames must be at least 1)")
    return [(int(a), int(b)) for a, b in zip(st[:k.value], en[:k.value])]


def write_chapter_exe(path, scene_changes, nframes, mute=None, only_muted=False):
    """chapter_exe's output file (CMAnalyze::readSceneChanges' input, passed on to join_logo_scp): SCPos lines, and with mute
    [(start, end)] (mute_sections) the "mute" lines in front of the scene changes they hold; only_muted drops every other scene change"""
    lib = binding.load()
    sc = np.ascontiguousarray(scene_changes, np.int32).reshape(-1)
    if mute is None:
        if only_muted:
            raise AmtError("write_chapter_exe: only_muted needs the mute sections")
        ok = lib.amtgpu_cm_write_chapter_exe(_p(sc), len(sc), int(nframes), str(path).encode())
    else:
        m = np.ascontiguousarray(mute, np.int32).reshape(-1, 2)
        st, en = np.ascontiguousarray(m[:, 0]), np.ascontiguousarray(m[:, 1])
        ok = lib.amtgpu_cm_write_chapter_exe_mute(_p(sc), len(sc), _p(st), _p(en), len(st), int(nframes), 1 if only_muted else 0, str(path).encode())
    if not ok:
        raise AmtError(f"write_chapter_exe({path}): refused (scene changes or sections unsorted, overlapping or outside the clip) or not writable")


RENDER_WEAVE, RENDER_BOB_TOP, RENDER_BOB_BOTTOM = 0, 1, 2
RENDER_FRAME = np.dtype([("kind", np.int32), ("top", np.int32), ("bottom", np.int32), ("ticks", np.int32)])      # AmtGpuRenderFrame
DEINT_LINE, DEINT_ADAPTIVE = 0, 1                                                                                # AMTGPU_DEINT_*


def kfm_render_plan(cadence, phase):
    """The pictures that go with the cadence decisions (self-specified): one RENDER_FRAME record per output frame,
    in the order of the durations file and with its ticks -- WEAVE(top, bottom) for film and progressive frames, BOB_TOP(n) then
    BOB_BOTTOM(n) for a 60i frame.  Source frame numbers are absolute."""
    cad = np.ascontiguousarray(cadence, np.uint8).reshape(-1)
    ph = np.ascontiguousarray(phase, np.uint8).reshape(-1)
    if len(cad) != len(ph):
        raise AmtError("kfm_render_plan: cadence and phase differ in length")
    lib = binding.load()
    out = np.zeros(2 * len(cad), RENDER_FRAME)
    k = C.c_int()
    if not lib.amtgpu_kfm_render_plan(_p(cad), _p(ph), len(cad), _p(out), len(out), C.byref(k)):
        raise AmtError("amtgpu_kfm_render_plan failed")
    return out[:k.value].copy()


def _surfaces_ref(clip):
    if isinstance(clip, DeviceSurfaces):
        return clip.ref()
    return DeviceSurfaces(clip.Y, clip.U, clip.V, clip.width, clip.height, clip.bits).ref()


def kfm_render(ctx: Context, src: "DeviceSurfaces | DeviceClip", plan, dst: "DeviceSurfaces | DeviceClip", src_first=0, clip_frames=None, thresh=-1,
               deint="line"):
    """Renders the plan's output frames (kfm_render_plan, or any RENDER_FRAME array) into dst's first len(plan) frames: woven film
    frames and bob-deinterlaced fields.  src holds frames [src_first, src_first + src.num_frames) of a clip of
    clip_frames frames (default: the batch ends the clip).  src and dst are planar clips or decoder surfaces IN KIND -- equal bits,
    interleaved and msb: NV12 in, NV12 out; P010 in, P010 out (V = None when interleaved); no layout is converted.  thresh >= 0: a
    missing row takes the average of its two temporal neighbours where they differ by at most thresh, which needs frame n - 1 / n + 1
    in the batch; the default -1 is the pure line-average bob.  thresh counts container units, or samples (container >> (16 - bits))
    when msb: interpolated rows are then computed on samples and stored with zero low bits, copied rows keep theirs.
    deint="adaptive" fills the missing rows of the 60i frames with the edge-directed, motion-adaptive rule instead (amtgpu_kfm_render_deint;
    DESIGN.md section 6d): still areas weave, moving areas interpolate along the edge.  It has no threshold (thresh must stay -1), reads
    frames n - 1 and n + 1 of every bob entry wherever the clip has them, and takes every pair in kind: planar LSB clips go through
    amtgpu_kfm_render_deint as before, interleaved or MSB-aligned surfaces (NV12, P010 / P012, planar MSB) through
    amtgpu_kfm_render_deint_surfaces, where U and V are planes of their own, the rule runs on samples (container >> (16 - bits) when msb),
    interpolated containers are stored with zero low bits and copied rows keep theirs.  Synchronises"""
    if deint not in ("line", "adaptive"):
        raise AmtError(f"kfm_render: deint is 'line' or 'adaptive', not {deint!r}")
    pl = np.ascontiguousarray(plan, RENDER_FRAME).reshape(-1)
    nsrc = src.num_frames
    if clip_frames is None:
        clip_frames = src_first + nsrc
    if len(pl) > dst.num_frames:
        raise AmtError(f"kfm_render: the plan has {len(pl)} output frames, dst holds {dst.num_frames}")
    s, d = _surfaces_ref(src), _surfaces_ref(dst)
    if deint == "adaptive":
        call = ctx.lib.amtgpu_kfm_render_deint_surfaces if s.interleaved or s.msb_aligned else ctx.lib.amtgpu_kfm_render_deint
        ctx.check(call(ctx.h, C.byref(s), int(src_first), nsrc, int(clip_frames), int(src.width), int(src.height), _p(pl), len(pl), DEINT_ADAPTIVE, int(thresh),
                       C.byref(d)), "kfm_render")
        return
    ctx.check(ctx.lib.amtgpu_kfm_render(ctx.h, C.byref(s), int(src_first), nsrc, int(clip_frames), int(src.width), int(src.height), _p(pl), len(pl),
                                        int(thresh), C.byref(d)), "kfm_render")


def temporal_nr(ctx: Context, src: "DeviceSurfaces | DeviceClip", dst: "DeviceSurfaces | DeviceClip", distance=3, threshold=1, interlaced=False, src_first=0,
                clip_frames=None, out_first=None, nout=None):
    """Temporal noise reduction, the reference's TemporalNRFilter byte for byte (amtgpu_temporal_nr): per luma pixel
    the mean of the window frames clamp(t - distance .. t + distance, 0, clip_frames - 1) whose |dY| + |dU| + |dV| against frame t is at
    most threshold << (bits - 8).  The defaults are the server's KTemporalNR(3, 1).  src holds frames [src_first, src_first +
    src.num_frames) of a clip of clip_frames frames (default: the batch ends the clip); output frames out_first .. out_first + nout - 1 go
    to dst's frames 0 .. nout - 1 (default: every frame whose window lies in the batch).  src and dst are planar clips or decoder
    surfaces IN KIND -- equal bits, interleaved and msb: NV12 in, NV12 out; P010 in, P010 out (V = None when interleaved); no layout is
    converted.  Interleaved or MSB-aligned surfaces go through amtgpu_temporal_nr_surfaces: the rule runs on samples (container >>
    (16 - bits) when msb, which the threshold counts), and every output container is the result << (16 - bits), its low bits zero.
    interlaced picks the chroma row of interlaced 4:2:0 and needs height % 4 == 0.  Synchronises.  Returns (out_first, nout)"""
    nsrc, d = src.num_frames, int(distance)
    if clip_frames is None:
        clip_frames = src_first + nsrc
    if out_first is None:
        out_first = src_first if src_first == 0 else src_first + d
    if nout is None:
        end = src_first + nsrc                       # one past the last output frame whose window the batch holds
        nout = max(0, (end if end == clip_frames else end - d) - out_first)
    if nout > dst.num_frames:
        raise AmtError(f"temporal_nr: {nout} output frames, dst holds {dst.num_frames}")
    s, t = _surfaces_ref(src), _surfaces_ref(dst)
    call = ctx.lib.amtgpu_temporal_nr_surfaces if s.interleaved or s.msb_aligned else ctx.lib.amtgpu_temporal_nr
    ctx.check(call(ctx.h, C.byref(s), int(src_first), nsrc, int(clip_frames), int(src.width), int(src.height), int(out_first), int(nout),
                   d, int(threshold), 1 if interlaced else 0, C.byref(t)), "temporal_nr")
    return int(out_first), int(nout)


RESIZE_KERNELS = {"blackman": 0, "lanczos": 1, "bilinear": 2}                                                       # AMTGPU_RESIZE_*


class Resizer:
    """Blackman / Lanczos / bilinear resize of clips in HBM, planar or decoder surfaces in kind (amtgpu_resize_*): the
    BlackmanResize(w, h) in front of KTemporalNR in the server's chain, integer and exact -- horizontal stage first into an intermediate
    the object owns, then vertical; every plane on its own, chroma (w/2, h/2) -> (w/2, h/2) with the same kernel.  src_size and dst_size are (width, height)
    of the luma plane, all four even.  taps None: the kernel's default (blackman 4, lanczos 3).  max_scratch_bytes bounds the
    intermediate, not the clip: a run works through its frames in rounds (None: the header's default, 64 MiB)."""

    def __init__(self, ctx: Context, src_size, dst_size, bits, kernel="blackman", taps=None, max_scratch_bytes=None):
        if kernel not in RESIZE_KERNELS:
            raise AmtError(f"Resizer: kernel is one of {sorted(RESIZE_KERNELS)}, not {kernel!r}")
        self.ctx, self.bits, self.kernel = ctx, int(bits), kernel
        (self.src_w, self.src_h), (self.dst_w, self.dst_h) = (int(v) for v in src_size), (int(v) for v in dst_size)
        self.h = ctx.lib.amtgpu_resize_create(ctx.h, self.src_w, self.src_h, self.dst_w, self.dst_h, self.bits, RESIZE_KERNELS[kernel],
                                              0 if taps is None else int(taps), 0 if max_scratch_bytes is None else int(max_scratch_bytes))
        ctx.check(self.h, "Resizer")

    def run(self, src: "DeviceSurfaces | DeviceClip", dst: "DeviceSurfaces | DeviceClip"):
        """frames 0 .. src.num_frames - 1 of src into the same frames of dst, both of the resizer's bits.  Planar LSB planes go to
        amtgpu_resize_run; where either is interleaved or MSB-aligned (NV12, P010 / P012 / P016, interleaved LSB, planar MSB) the pair
        goes to amtgpu_resize_run_surfaces and must be in kind: the rule runs on container >> shift, U and V each on its own, and every
        destination container is result << shift with zero low bits.  Synchronises.  Returns the number of frames"""
        n = src.num_frames
        if n > dst.num_frames:
            raise AmtError(f"Resizer: {n} frames, dst holds {dst.num_frames}")
        if (int(src.width), int(src.height)) != (self.src_w, self.src_h) or (int(dst.width), int(dst.height)) != (self.dst_w, self.dst_h):
            raise AmtError(f"Resizer: made for {self.src_w}x{self.src_h} -> {self.dst_w}x{self.dst_h}, got {src.width}x{src.height} -> {dst.width}x{dst.height}")
        s, t = _surfaces_ref(src), _surfaces_ref(dst)
        in_kind = s.interleaved or s.msb_aligned or t.interleaved or t.msb_aligned
        run = self.ctx.lib.amtgpu_resize_run_surfaces if in_kind else self.ctx.lib.amtgpu_resize_run
        self.ctx.check(run(self.h, C.byref(s), C.byref(t), n), "Resizer")
        return n

    def program(self, plane, axis):
        """(K, start[D], coeff[D][K]) of plane 0 (luma) / 1 (chroma), axis 0 (horizontal) / 1 (vertical), as numpy int32"""
        k = C.c_int()
        self.ctx.check(self.ctx.lib.amtgpu_resize_get_program(self.h, int(plane), int(axis), C.byref(k), None, None), "Resizer")
        D = ((self.dst_h if axis else self.dst_w) >> 1) if plane else (self.dst_h if axis else self.dst_w)
        start, coeff = np.zeros(D, np.int32), np.zeros((D, k.value), np.int32)
        self.ctx.check(self.ctx.lib.amtgpu_resize_get_program(self.h, int(plane), int(axis), C.byref(k), _p(start), _p(coeff)), "Resizer")
        return k.value, start, coeff

    def close(self):
        if self.h:
            self.ctx.lib.amtgpu_resize_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Debander:
    """Deband of clips in HBM, planar or decoder surfaces in kind (amtgpu_deband_*): the KDeband(25, 1, 2, true) behind KTemporalNR
    in the server's chain, integer and exact.  Per pixel up to four references at the offsets of a table that is static over frames
    (a hash of the position, the plane and `seed`; |dx|, |dy| <= min(radius, distance to the plane's edge), chroma at radius >> 1):
    sample 0 takes the first reference, 1 the mean of a pair, 2 the mean of two pairs at right angles; blur_first compares the mean with
    the pixel, otherwise every reference must lie within threshold << (bits - 8) of it.  Every plane and every frame on its own.  size
    is (width, height) of the luma plane, both even.  The arguments' order and defaults are the server's call."""

    def __init__(self, ctx: Context, size, bits, radius=25, threshold=1, sample=2, blur_first=True, seed=0):
        self.ctx, self.bits = ctx, int(bits)
        self.width, self.height = (int(v) for v in size)
        self.h = ctx.lib.amtgpu_deband_create(ctx.h, self.width, self.height, self.bits, int(radius), int(threshold), int(sample), 1 if blur_first else 0,
                                              int(seed) & 0xFFFFFFFF)
        ctx.check(self.h, "Debander")

    def run(self, src: "DeviceSurfaces | DeviceClip", dst: "DeviceSurfaces | DeviceClip"):
        """frames 0 .. src.num_frames - 1 of src into the same frames of dst, both of the debander's size and bits; dst must not overlap
        src.  Planar LSB planes go to amtgpu_deband_run; where either is interleaved or MSB-aligned (NV12, P010 / P012 / P016,
        interleaved LSB, planar MSB) the pair goes to amtgpu_deband_run_surfaces and must be in kind: the rule runs on container >>
        shift, U and V each on its own with its own table, and every destination container is result << shift with zero low bits.
        Synchronises.  Returns the number of frames"""
        n = src.num_frames
        if n > dst.num_frames:
            raise AmtError(f"Debander: {n} frames, dst holds {dst.num_frames}")
        for c in (src, dst):
            if (int(c.width), int(c.height)) != (self.width, self.height):
                raise AmtError(f"Debander: made for {self.width}x{self.height}, got {c.width}x{c.height}")
        s, t = _surfaces_ref(src), _surfaces_ref(dst)
        in_kind = s.interleaved or s.msb_aligned or t.interleaved or t.msb_aligned
        run = self.ctx.lib.amtgpu_deband_run_surfaces if in_kind else self.ctx.lib.amtgpu_deband_run
        self.ctx.check(run(self.h, C.byref(s), C.byref(t), n), "Debander")
        return n

    def _plane_shape(self, plane):
        return (self.height >> 1, self.width >> 1) if plane else (self.height, self.width)

    def offsets(self, plane):
        """(dx, dy) of plane 0 (Y) / 1 (U) / 2 (V), each (Hp, Wp) numpy int8"""
        dx, dy = np.zeros(self._plane_shape(plane), np.int8), np.zeros(self._plane_shape(plane), np.int8)
        self.ctx.check(self.ctx.lib.amtgpu_deband_get_offsets(self.h, int(plane), _p(dx), _p(dy)), "Debander")
        return dx, dy

    def set_offsets(self, plane, dx, dy):
        """replaces one plane's table; refused where an entry exceeds min(radius, distance to the plane's edge)"""
        if plane not in (0, 1, 2):
            raise AmtError(f"Debander: plane is 0 (Y), 1 (U) or 2 (V), not {plane!r}")
        dx, dy = np.ascontiguousarray(dx, np.int8), np.ascontiguousarray(dy, np.int8)
        if dx.shape != self._plane_shape(plane) or dy.shape != dx.shape:
            raise AmtError(f"Debander: plane {plane} takes tables of {self._plane_shape(plane)}, got {dx.shape} and {dy.shape}")
        self.ctx.check(self.ctx.lib.amtgpu_deband_set_offsets(self.h, int(plane), _p(dx), _p(dy)), "Debander")

    def close(self):
        if self.h:
            self.ctx.lib.amtgpu_deband_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def edge_level(ctx: Context, src: "DeviceSurfaces | DeviceClip", dst: "DeviceSurfaces | DeviceClip", strength=16, threshold=10, repair=2):
    """Edge level of clips in HBM (amtgpu_edgelevel): the KEdgeLevel(16, 10, 2) behind KDeband in the server's chain,
    integer and exact.  Self-specified ("parity unpinned"): the rule is this project's, its constants are the specification's own, and no
    real footage has been judged.  Per interior luma pixel the line of five -- the column where its range exceeds the row's, else the row
    -- is levelled towards its nearer end, e = c + (((c - (max + min >> 1)) * strength) >> 4) clamped into [min, max], unless the line is
    flat (range <= threshold << (bits - 8)), sharp already (4 step >= 3 range) or too blurred (8 step <= 3 range); repair r > 0 then
    clamps e between the r-th smallest and the r-th largest of the 3 x 3 around the pixel.  The two outermost rows and columns and
    both chroma planes are copied.  Frames 0 .. src.num_frames - 1 of src go into the same frames of dst; both are planar LSB clips of
    one size and depth and must not overlap.  The arguments' order and defaults are the server's call.  Synchronises.  Returns the
    number of frames"""
    n = src.num_frames
    if n > dst.num_frames:
        raise AmtError(f"edge_level: {n} frames, dst holds {dst.num_frames}")
    if (int(src.width), int(src.height)) != (int(dst.width), int(dst.height)):
        raise AmtError(f"edge_level: src is {src.width}x{src.height}, dst {dst.width}x{dst.height}")
    s, t = _surfaces_ref(src), _surfaces_ref(dst)
    ctx.check(ctx.lib.amtgpu_edgelevel(ctx.h, C.byref(s), C.byref(t), int(src.width), int(src.height), n, int(strength), int(threshold), int(repair)),
              "edge_level")
    return n
