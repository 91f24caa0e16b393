"""The temporal noise reduction (temporal_nr, csrc/temporal_nr_kernels.hip) measured on an MI355X beside a whole-frame copy; writes
profiles/temporal_nr.json.

  1920x1080 at 8 and at 10 bits, 1 024 frames resident in HBM (3.2 / 6.4 GB; with the destination far above the 256 MiB Infinity
  Cache), temporal_distance 3, threshold 1 (the server's KTemporalNR(3, 1)).  The clip is a still random picture with per-frame noise of
  -1 .. 1 on every sample, so that windows do pass frames; the kernel's work does not depend on the samples (a select, not a branch).
  The comparator is kfm_render with an all-30p plan on the same buffers -- a whole-frame copy, each frame read once and written once,
  which are the filter's algorithmic bytes too -- alternating with the filter in the same run.  Times are the context's HIP events around
  the one kernel launch of a call (Context.profile), median [min - max] of 7 after 2 warm-up calls.

  From the ISA (the file compiled as build.py compiles it): each form's registers, and the vector instructions in the two window loops
  of the 16-byte forms.  With them a lower bound of the arithmetic's time: lanes' cells / 64 wave-instructions per loop instruction and
  window frame, each 4 cycles of a SIMD's 16 lanes wide vector unit (packed and plain operations alike; dual issue and the scalar unit
  not counted), over 256 CUs x 4 SIMDs at 2.4 GHz -- to say which of the two bounds, memory or arithmetic, the kernel runs against.

  Output frames 0, the middle one and the last are checked against the numpy restatement (tests/temporal_nr_ref.py) before any timing.

    python tools/temporal_nr_bench.py [--out profiles/temporal_nr.json] [--frames 1024]
There is no CPU path: without a GPU this fails."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kfm_render_bench import H, HBM_PEAK, REPS, W, WARMUP, kernel_ms, rates, spread  # noqa: E402

CUS, SIMDS_PER_CU, CLOCK_HZ, CYCLES_PER_WAVE_VALU = 256, 4, 2.4e9, 4
D, THRESHOLD = 3, 1
FORMS = {"IhLb1E": "8-bit containers, 16-byte lanes", "IhLb0E": "8-bit containers, container by container",
         "ItLb1E": "16-bit containers, 16-byte lanes", "ItLb0E": "16-bit containers, container by container"}


def kernel_isa():
    """{form: VGPRs, and for the 16-byte forms the vector instructions of the count loop and of the sum loop}"""
    from test_isa_guards import kernels_of
    from test_isa_surfaces import compile_file
    asm = compile_file("temporal_nr_kernels.hip")
    res = {}
    for name, k in kernels_of(asm).items():
        tag = re.search(r"temporal_nr_kernel(I[ht]Lb[01]E)", name).group(1)
        res[FORMS[tag]] = {"vgprs": k["meta"]["vgpr_count"]}
        if tag.endswith("Lb1E"):
            text = asm[asm.index("\n" + name + ":"):]
            loops = re.findall(r"^(\.LBB\d+_\d+):[^\n]*Inner Loop Header[^\n]*\n(.*?)^\s+s_cbranch_\w+ \1$", text, re.M | re.S)[:2]
            assert len(loops) == 2, (name, len(loops))
            valu = [sum(bool(re.match(r"\s+v_", l)) for l in body.split("\n")) for _, body in loops]
            res[FORMS[tag]].update({"count_loop_vector_instructions": valu[0], "sum_loop_vector_instructions": valu[1]})
    return res


def noisy_clip(A, torch, n, bits, seed):
    """a still random picture (away from the range's ends) with noise of -1 .. 1 on every sample of every frame"""
    dt = torch.uint8 if bits <= 8 else torch.int16
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)

    def mk(h, w):
        p = torch.randint(0, 3, (n, h, w), dtype=dt, device="cuda", generator=gen)
        p += torch.randint(1, (1 << bits) - 3, (1, h, w), dtype=dt, device="cuda", generator=gen)
        return p
    return A.DeviceClip(mk(H, W), mk(H // 2, W // 2), mk(H // 2, W // 2), W, H, bits)


def empty_clip(A, torch, n, bits):
    dt = torch.uint8 if bits <= 8 else torch.int16
    mk = lambda h, w: torch.empty((n, h, w), dtype=dt, device="cuda")
    return A.DeviceClip(mk(H, W), mk(H // 2, W // 2), mk(H // 2, W // 2), W, H, bits)


def vector_form(clip_, dst, es):
    """temporal_nr_vec16 (csrc/lane_rule.h) on these tensors"""
    bits = lambda t: t.data_ptr() | (t.stride(0) * es) | (t.stride(1) * es)
    return (bits(clip_.Y) | bits(dst.Y)) % 16 == 0 and (bits(clip_.U) | bits(clip_.V) | bits(dst.U) | bits(dst.V)) % 8 == 0


def check_frames(np, R, src, dst, bits):
    dt = np.uint8 if bits <= 8 else np.uint16
    host = lambda t: t.cpu().numpy().view(dt)
    n = src.num_frames
    frames = (0, n // 2, n - 1)
    for t in frames:
        win = R.window(t, D, n)
        lo = min(win)
        planes = tuple(host(p[lo:max(win) + 1]) for p in (src.Y, src.U, src.V))
        want = R.filter_frame(planes, t - lo, D, THRESHOLD, bits, win=[f - lo for f in win])
        # the filter has work to do (at a clip end the centre frame is most of its own window, and the mean rounds back to it)
        assert int(want[3].max()) == 2 * D + 1 and (len(set(win)) < len(win) or float(np.mean(want[0] != planes[0][t - lo])) > 0.05)
        for g, w_ in zip((dst.Y, dst.U, dst.V), want):
            assert np.array_equal(host(g[t]), w_), ("output frame", t)
    return len(frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_nr.json"))
    ap.add_argument("--frames", type=int, default=1024)
    args = ap.parse_args()
    import numpy as np
    import torch
    import amatsukaze_amd as A
    import temporal_nr_ref as R
    N = args.frames
    isa = kernel_isa()
    ctx = A.Context(0)
    ctx.profile(True)
    res = {"what": "temporal_nr_kernel beside kfm_render_kernel with an all-30p plan (a whole-frame copy), %dx%d, %d frames in HBM, temporal_distance %d, "
                   "threshold %d; HIP events around the launch, median [min - max] of %d after %d warm-up calls, the two alternating on the same "
                   "buffers; bytes are algorithmic: each frame read once and written once (tools/temporal_nr_bench.py)" % (W, H, N, D, THRESHOLD, REPS, WARMUP),
           "device": torch.cuda.get_device_name(0), "peak_TB_per_s": 8.0, "isa": isa, "cases": []}
    plan = A.kfm_render_plan([2] * N, [0] * N)
    assert len(plan) == N
    for bits in (8, 10):
        es = 1 if bits <= 8 else 2
        frame_bytes = (W * H + 2 * (W // 2) * (H // 2)) * es
        nbytes = 2.0 * N * frame_bytes
        src = noisy_clip(A, torch, N, bits, seed=31 + bits)
        dst = empty_clip(A, torch, N, bits)
        vec = vector_form(src, dst, es)
        form = "%d-bit containers, %s" % (8 * es, "16-byte lanes" if vec else "container by container")
        calls = {"temporal_nr": ("temporal_nr_kernel", lambda: A.temporal_nr(ctx, src, dst, D, THRESHOLD)),
                 "copy (kfm_render, all-30p)": ("kfm_render_kernel", lambda: A.kfm_render(ctx, src, plan, dst))}
        calls["temporal_nr"][1]()
        checked = check_frames(np, R, src, dst, bits)
        ms = {name: [] for name in calls}
        for i in range(WARMUP + REPS):
            for name, (kernel, call) in calls.items():
                t = kernel_ms(ctx, kernel, call)
                if i >= WARMUP:
                    ms[name].append(t)
        copy = spread(ms["copy (kfm_render, all-30p)"])
        for name, (kernel, _) in calls.items():
            t = spread(ms[name])
            case = {"call": name, "kernel": kernel, "bits": bits, "frames": N, "algorithmic_bytes": nbytes, "ms": t, **rates(nbytes, t)}
            if name == "temporal_nr":
                px = 16 // es                                                  # luma columns of a cell of the 16-byte forms
                cells = N * (H // 2) * -(-W // px)
                case.update({"form": form, "vgprs": isa[form]["vgprs"], "frames_checked_against_numpy": checked,
                             "ratio_to_copy": t["median"] / copy["median"], "ranges_apart_from_copy": bool(t["min"] > copy["max"] or t["max"] < copy["min"])})
                if vec:
                    per_frame = isa[form]["count_loop_vector_instructions"] + isa[form]["sum_loop_vector_instructions"]
                    valu_ms = cells / 64 * per_frame * (2 * D + 1) * CYCLES_PER_WAVE_VALU / (CUS * SIMDS_PER_CU * CLOCK_HZ) * 1e3
                    mem_ms = nbytes / HBM_PEAK * 1e3
                    case.update({"vector_instructions_per_luma_pixel": per_frame * (2 * D + 1) / (2 * px),
                                 "arithmetic_lower_bound_ms": valu_ms, "memory_lower_bound_ms_at_8TBps": mem_ms,
                                 "measured_over_arithmetic_bound": t["median"] / valu_ms, "measured_over_memory_bound": t["median"] / mem_ms,
                                 "nearer_bound": "arithmetic" if valu_ms > mem_ms else "memory"})
            res["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
        del src, dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
