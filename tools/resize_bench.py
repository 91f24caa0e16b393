"""The resize (Resizer, csrc/resize_kernels.hip) measured on an MI355X beside a whole-frame copy; writes profiles/resize.json.

  1920x1080 -> 1280x720 at 8 and at 10 bits, 1 024 frames resident in HBM, Blackman taps 4 (the server's BlackmanResize(1280, 720)),
  the default scratch (rounds of as many frames as fit 64 MiB of intermediate).  The comparator is kfm_render with an all-30p plan on
  source-sized buffers -- a whole-frame copy -- alternating with the resize in the same run.  Times are the context's HIP events around
  the kernel launches of a call (Context.profile; the resize launches two kernels per round, summed per stage), median [min - max] of 7
  after 2 warm-up calls.

  Bytes: algorithmic = the source read once plus the destination written once; and, separately, with the intermediate written by the
  horizontal stage and read by the vertical one.  Both over the total time, as shares of 8 TB/s and beside the guide's copy figure.

  From the ISA (the file compiled as build.py compiles it), for the forms the timed case runs: the vector instructions per output sample
  of each stage -- horizontal: the tap section of the row loop (one output sample per lane and row) plus one pass of the 16-byte staging
  loop; vertical: the four-tap body of the row walk per tap and sample, times K, plus the store section per sample -- and the issue-rate
  bound they give, computed as DESIGN.md section 10 does it: wave-instructions x 4 cycles over 256 CUs x 4 SIMDs at 2.4 GHz, idle lanes
  of partly filled waves counted as issued, dual issue and the scalar unit not counted.

  Output frames 0, the middle one and the last are compared with the numpy restatement (tests/resize_ref.py) before any timing.

    python tools/resize_bench.py [--out profiles/resize.json] [--frames 1024]
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

DW, DH = 1280, 720
CUS, SIMDS_PER_CU, CLOCK_HZ, CYCLES_PER_WAVE_VALU = 256, 4, 2.4e9, 4
ROWS_PER_WAVE = 16                               # kResizeRows


def blocks_of(body):
    """the kernel's basic blocks in layout order: lists of instruction lines"""
    out, cur = [], []
    for l in body:
        if re.match(r"^\.LBB\d+_\d+:", l.strip()):
            out.append(cur)
            cur = []
        else:
            cur.append(l.strip())
    out.append(cur)
    return [b for b in out if b]


def valu(lines):
    return sum(l.startswith("v_") for l in lines)


def kernel_isa(K):
    """{form: registers and the vector instructions of its hot sections} for the forms a K-tap resize runs"""
    from test_isa_guards import kernels_of
    from test_isa_surfaces import compile_file
    kr = 8 if K <= 8 else 12 if K <= 12 else 16 if K <= 16 else 0
    res = {}
    for name, k in kernels_of(compile_file("resize_kernels.hip")).items():
        body = [l.strip() for l in k["body"]]
        for t, es in (("h", 1), ("t", 2)):
            if f"resize_h_kernelI{t}Li{kr}E" in name:
                first = next(i for i, l in enumerate(body) if l.startswith("ds_read"))
                last = next(i for i, l in enumerate(body) if i > first and re.match(r"global_store_(byte|short)", l))
                stage = next(b for b in blocks_of(body) if any(l.startswith("ds_write_b128") for l in b))
                res[f"horizontal, {8 * es}-bit containers, {kr} taps in registers"] = {
                    "vgprs": k["meta"]["vgpr_count"], "tap_section_vector_instructions": valu(body[first:last + 1]),
                    "tap_section_lds_reads": sum(l.startswith("ds_read") for l in body[first:last + 1]),
                    "staging_pass_vector_instructions": valu(stage)}
            if f"resize_v_kernelI{t}Lb1E" in name:
                bl = blocks_of(body)
                walk = max(bl, key=lambda b: sum(l.startswith("global_load_dwordx4") for l in b))
                taps = sum(l.startswith("global_load_dwordx4") for l in walk)
                store = next(b for b in bl if any(l.startswith("global_store_dwordx4") for l in b))
                res[f"vertical, {8 * es}-bit containers, 16-byte lanes"] = {
                    "vgprs": k["meta"]["vgpr_count"], "walk_body_taps": taps, "walk_body_vector_instructions": valu(walk),
                    "store_section_vector_instructions": valu(store), "samples_per_lane": 16 // es}
    return res


def clip(A, torch, n, w, h, bits, seed=None):
    dt = torch.uint8 if bits <= 8 else torch.int16
    if seed is None:
        mk = lambda hh, ww: torch.empty((n, hh, ww), dtype=dt, device="cuda")
    else:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed)
        mk = lambda hh, ww: torch.randint(0, 1 << bits, (n, hh, ww), dtype=dt, device="cuda", generator=gen)
    return A.DeviceClip(mk(h, w), mk(h // 2, w // 2), mk(h // 2, w // 2), w, h, bits)


def check_frames(np, R, src, dst, bits):
    dt = np.uint8 if bits <= 8 else np.uint16
    host = lambda t: t.cpu().numpy().view(dt)
    n = src.num_frames
    frames = sorted({0, n // 2, n - 1})
    for f in frames:
        want = R.resize_clip(tuple(host(p[f:f + 1]) for p in (src.Y, src.U, src.V)), DW, DH, bits)
        for g, w_ in zip((dst.Y, dst.U, dst.V), want):
            assert np.array_equal(host(g[f:f + 1]), w_), ("output frame", f)
    return len(frames)


def stage_ms(ctx, call):
    """HIP-event times of the two stages' launches inside call(): ({kernel: ms}, launches per stage)"""
    names = ("resize_h_kernel", "resize_v_kernel")
    before = {k: ctx.profile_report().get(k, (0, 0.0)) for k in names}
    call()
    after = {k: ctx.profile_report()[k] for k in names}
    launches = {after[k][0] - before[k][0] for k in names}
    assert len(launches) == 1
    return {k: after[k][1] - before[k][1] for k in names}, launches.pop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize.json"))
    ap.add_argument("--frames", type=int, default=1024)
    args = ap.parse_args()
    import numpy as np
    import torch
    import amatsukaze_amd as A
    import resize_ref as R
    N = args.frames
    K = R.program(W, DW)[0]
    assert K == R.program(H, DH)[0] == R.program(W // 2, DW // 2)[0] == R.program(H // 2, DH // 2)[0] == 12
    isa = kernel_isa(K)
    ctx = A.Context(0)
    ctx.profile(True)
    res = {"what": "Resizer %dx%d -> %dx%d (Blackman, taps 4, K %d), %d frames in HBM, default scratch, beside kfm_render_kernel with an all-30p plan on "
                   "source-sized buffers (a whole-frame copy); HIP events around the launches, median [min - max] of %d after %d warm-up calls, "
                   "the two alternating in the same run (tools/resize_bench.py).  A packed or dot multiply form was not tried: not measured"
                   % (W, H, DW, DH, K, N, REPS, WARMUP),
           "device": torch.cuda.get_device_name(0), "peak_TB_per_s": 8.0, "isa": isa, "cases": []}
    plan = A.kfm_render_plan([2] * N, [0] * N)
    assert len(plan) == N
    slots = CUS * SIMDS_PER_CU * CLOCK_HZ
    for bits in (8, 10):
        es = 1 if bits <= 8 else 2
        src_frame, dst_frame, mid_frame = (W * H * 3 // 2) * es, (DW * DH * 3 // 2) * es, (DW * H * 3 // 2) * es
        src = clip(A, torch, N, W, H, bits, seed=41 + bits)
        dst = clip(A, torch, N, DW, DH, bits)
        copy_dst = clip(A, torch, N, W, H, bits)
        rz = A.Resizer(ctx, (W, H), (DW, DH), bits)
        rz.run(src, dst)
        checked = check_frames(np, R, src, dst, bits)
        ms = {"horizontal": [], "vertical": [], "total": [], "copy": []}
        launches = None
        for i in range(WARMUP + REPS):
            t, launches = stage_ms(ctx, lambda: rz.run(src, dst))
            c = kernel_ms(ctx, "kfm_render_kernel", lambda: A.kfm_render(ctx, src, plan, copy_dst))
            if i >= WARMUP:
                ms["horizontal"].append(t["resize_h_kernel"]); ms["vertical"].append(t["resize_v_kernel"])
                ms["total"].append(t["resize_h_kernel"] + t["resize_v_kernel"]); ms["copy"].append(c)
        sp = {k: spread(v) for k, v in ms.items()}
        alg, with_mid = float(N) * (src_frame + dst_frame), float(N) * (src_frame + dst_frame + 2 * mid_frame)
        hi, vi = isa[f"horizontal, {8 * es}-bit containers, 12 taps in registers"], isa[f"vertical, {8 * es}-bit containers, 16-byte lanes"]
        # wave-instructions: horizontal -- every (run of 64 columns, row) of the intermediate issues the tap section and one staging pass;
        # vertical -- every (64-lane chunk, output row) issues K taps of the walk body and the store section
        px = 16 // es
        h_waves = sum(-(-dw // 64) * sh for dw, sh in ((DW, H), (DW // 2, H // 2), (DW // 2, H // 2))) * N
        v_waves = sum(-(-(-(-dw // px)) // 64) * dh for dw, dh in ((DW, DH), (DW // 2, DH // 2), (DW // 2, DH // 2))) * N
        h_per_wave = hi["tap_section_vector_instructions"] + hi["staging_pass_vector_instructions"]
        v_per_wave = vi["walk_body_vector_instructions"] / vi["walk_body_taps"] * K + vi["store_section_vector_instructions"]
        h_bound = h_waves * h_per_wave * CYCLES_PER_WAVE_VALU / slots * 1e3
        v_bound = v_waves * v_per_wave * CYCLES_PER_WAVE_VALU / slots * 1e3
        mid_samples, out_samples = N * DW * H * 3 // 2, N * DW * DH * 3 // 2
        mem_alg_ms, mem_mid_ms = alg / HBM_PEAK * 1e3, with_mid / HBM_PEAK * 1e3
        case = {"bits": bits, "frames": N, "launches_per_stage": launches, "frames_checked_against_numpy": checked,
                "ms": sp,
                "algorithmic_bytes": alg, "algorithmic": rates(alg, sp["total"]),
                "bytes_with_intermediate": with_mid, "with_intermediate": rates(with_mid, sp["total"]),
                "horizontal_stage": {"bytes": float(N) * (src_frame + mid_frame), **rates(float(N) * (src_frame + mid_frame), sp["horizontal"]),
                                     "vector_instructions_per_output_sample": h_per_wave * h_waves * 64 / mid_samples,
                                     "vector_instructions_per_wave_and_row": h_per_wave, "issue_rate_bound_ms": h_bound},
                "vertical_stage": {"bytes": float(N) * (mid_frame + dst_frame), **rates(float(N) * (mid_frame + dst_frame), sp["vertical"]),
                                   "vector_instructions_per_output_sample": v_per_wave * v_waves * 64 / out_samples,
                                   "vector_instructions_per_wave_and_row": v_per_wave, "issue_rate_bound_ms": v_bound},
                "issue_rate_bound_ms": h_bound + v_bound, "memory_bound_ms_at_8TBps_algorithmic": mem_alg_ms,
                "memory_bound_ms_at_8TBps_with_intermediate": mem_mid_ms,
                "larger_bound": "issue rate" if h_bound + v_bound > mem_mid_ms else "memory",
                "measured_over_issue_rate_bound": sp["total"]["median"] / (h_bound + v_bound),
                "measured_over_memory_bound_with_intermediate": sp["total"]["median"] / mem_mid_ms,
                "copy": {"bytes": 2.0 * N * src_frame, **rates(2.0 * N * src_frame, sp["copy"])},
                "ratio_to_copy": sp["total"]["median"] / sp["copy"]["median"]}
        res["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        rz.close()
        del src, dst, copy_dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
