"""The deband (Debander, csrc/deband_kernels.hip) measured on an MI355X beside a whole-frame copy; writes profiles/deband.json.

  1920x1080 at 8 and at 14 bits, 1 024 frames resident in HBM, radius 25, threshold 1, sample 2, blur_first (the server's
  KDeband(25, 1, 2, true)), one launch per call.  The comparator is kfm_render with an all-30p plan on the same source and a buffer of
  the destination's size -- a whole-frame copy -- alternating with the deband in the same run.  Times are the context's HIP events
  around the kernel launch of a call (Context.profile), median [min - max] of 7 after 2 warm-up calls.

  Bytes: algorithmic = the source read once plus the destination written once; and, separately, with the halo the tiles re-read and
  the two offset tables every frame reads (static over frames: caches serve them), as the kernel requests them.

  From the ISA (the file compiled as build.py compiles it), for the 16-byte form the timed case runs: the vector instructions and LDS
  reads of the row loop of sample 2 with blur_first, per lane step (16 / es pixels), and the three bounds they give --
    issue rate: wave-instructions x 4 cycles over 256 CUs x 4 SIMDs at 2.4 GHz, as DESIGN.md section 10 counts (idle lanes of partly
      filled waves counted as issued, dual issue and the scalar unit not counted);
    LDS: the cycles of the LDS array per CU from the guide's model -- a container-wide read is served in two groups of 32 lanes, one
      cycle per distinct dword on the busiest of 32 banks -- evaluated on the very offsets of the timed table, plus 4 cycles per 16-byte
      centre read and 13 per 16-byte staging store; a model, not a counter: no PMC run was made (not measured);
    bytes: the algorithmic bytes at 8 TB/s.
  The global-gather alternative (references loaded from HBM / L2 without staging) was not built: not measured.

  Output frames 0, the middle one and the last are compared with the numpy restatement (tests/deband_ref.py) before any timing.

    python tools/deband_bench.py [--out profiles/deband.json] [--frames 1024]
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
from resize_bench import blocks_of, clip, valu  # noqa: E402

RADIUS, THRESHOLD, SAMPLE, BLUR_FIRST, SEED = 25, 1, 2, True, 0
TW, TH, HALO = 128, 96, 31                       # kDebandTileW, kDebandTileH, kDebandHalo (csrc/kernels.hpp)
CUS, SIMDS_PER_CU, CLOCK_HZ, CYCLES_PER_WAVE_VALU = 256, 4, 2.4e9, 4
LDS_READ128_CYCLES, LDS_WRITE128_CYCLES = 4, 13


def lds_pitch(es):
    return ((TW + 2 * HALO) * es + 30) & ~15


def kernel_isa():
    """{form: registers, LDS and the instructions of the row loop the timed case runs} for the two 16-byte forms"""
    from test_isa_guards import kernels_of
    from test_isa_surfaces import compile_file
    asm = compile_file("deband_kernels.hip")
    lds = {re.search(r"\.name:\s+(\S+)", m.group(0)).group(1): int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", m.group(0)).group(1))
           for m in re.finditer(r"- \.agpr_count:.*?\n(?=  - \.agpr_count:|\.\.\.|amdhsa\.target)", asm, re.S)}
    res = {}
    for name, k in kernels_of(asm).items():
        for t, es in (("h", 1), ("t", 2)):
            if f"deband_kernelI{t}Lb1E" not in name:
                continue
            px, read = 16 // es, "ds_read_u8" if es == 1 else "ds_read_u16"
            body = [l.strip() for l in k["body"]]
            # the row loops of sample 2 hold four references per pixel; blur_first's is the one without the per-reference comparisons
            loops = [b for b in blocks_of(body) if sum(l.startswith(read) for l in b) == 4 * px]
            assert len(loops) == 2, (name, len(loops))
            loop = min(loops, key=valu)
            res[f"{8 * es}-bit containers, 16-byte lanes"] = {
                "vgprs": k["meta"]["vgpr_count"], "lds_bytes": lds[name], "pixels_per_lane_step": px,
                "row_loop_vector_instructions": valu(loop), "row_loop_reference_reads": 4 * px,
                "row_loop_instructions": len(loop), "row_loop_full_width_multiplies": sum(l.startswith("v_mul_lo_u32") for l in loop)}
    return res


def tiles_of(w, h):
    return [(x0, y0) for y0 in range(0, h, TH) for x0 in range(0, w, TW)]


def work_model(np, R, es):
    """per frame, from the geometry and the very table the timed object holds: wave steps of the row loops, LDS-array cycles of the
    reference reads under the bank model, of the centre reads and of the staging stores, and the bytes the kernel requests"""
    px, lpr = 16 // es, TW // (16 // es)
    rpw = 64 // lpr                               # rows of a wave's step
    pitch = lds_pitch(es)
    wave_steps = ref_cycles = centre_cycles = stage_cycles = 0
    staged = table = 0
    for p in range(3):
        pw, ph = R.plane_size(p, W, H)
        rp = R.plane_radius(p, RADIUS)
        dx, dy = (a.astype(np.int64) for a in R.table(p, pw, ph, rp, SEED))
        # LDS byte address of every reference, relative to its tile's span (the bank pattern only needs it modulo 128)
        yy, xx = np.arange(ph)[:, None], np.arange(pw)[None, :]
        x0, y0 = xx // TW * TW, yy // TH * TH
        ox, sy0 = np.maximum(x0 - rp, 0) // px * px, np.maximum(y0 - rp, 0)
        centre = (yy - sy0) * pitch + (xx - ox) * es
        refs = [centre + dy * pitch + dx * es, centre - dy * pitch - dx * es, centre + dx * pitch - dy * es, centre - dx * pitch + dy * es]
        for tx0, ty0 in tiles_of(pw, ph):
            rows, cols = min(TH, ph - ty0), min(TW, pw - tx0)
            steps = -(-rows // rpw)               # wave steps of this tile: every lane row group of 64 lanes, idle lanes included
            wave_steps += steps
            centre_cycles += steps * LDS_READ128_CYCLES
            srows = min(ty0 + TH + rp, ph) - max(ty0 - rp, 0)
            sx0 = max(tx0 - rp, 0) // px * px
            pieces = -(-(min(tx0 + TW + rp, pw) - sx0) // px)
            stage_cycles += -(-srows * pieces // 64) * LDS_WRITE128_CYCLES + 0 * cols
            staged += srows * pieces * 16
            table += 2 * rows * (-(-cols // px) * px)
        # the reference reads: lanes of a wave are lpr cells of rpw rows; pixel j of each cell in one instruction.  Group the plane
        # into (wave step, j) instructions and their two halves of 32 lanes, count distinct dwords on the busiest bank
        ph_pad, pw_pad = -(-ph // TH) * TH, -(-pw // TW) * TW
        for a in refs:
            full = np.full((ph_pad, pw_pad), -1, np.int64)
            full[:ph, :pw] = a // 4
            # (tile row, step, row of wave, tile column, cell, pixel) -> instructions x lanes
            v = full.reshape(ph_pad // TH, TH // rpw, rpw, pw_pad // TW, lpr, px).transpose(0, 1, 3, 5, 2, 4).reshape(-1, 2, 32)
            for half in range(2):
                g = v[:, half, :]
                live = g >= 0
                bank = np.where(live, g % 32, 0)
                # distinct dwords per bank: sort by (bank, dword) and count changes
                key = np.where(live, bank * (1 << 40) + g, -1)
                key.sort(axis=1)
                new = np.ones_like(key, bool)
                new[:, 1:] = key[:, 1:] != key[:, :-1]
                new &= key >= 0
                kb = np.where(key >= 0, key >> 40, 32)
                busiest = np.zeros(len(key), np.int64)
                for b in range(32):
                    busiest = np.maximum(busiest, (new & (kb == b)).sum(axis=1))
                ref_cycles += int(busiest.sum())
    return {"wave_steps": wave_steps, "reference_read_cycles": ref_cycles, "centre_read_cycles": centre_cycles, "staging_store_cycles": stage_cycles,
            "staged_bytes": staged, "table_bytes": table}


def check_frames(np, R, src, dst, bits):
    dt = np.uint8 if bits <= 8 else np.uint16
    host = lambda t: t.cpu().numpy().view(dt)
    n = src.num_frames
    frames = sorted({0, n // 2, n - 1})
    for f in frames:
        want = R.filter_clip(tuple(host(p[f:f + 1]) for p in (src.Y, src.U, src.V)), bits, RADIUS, THRESHOLD, SAMPLE, BLUR_FIRST, SEED)
        for g, w_ in zip((dst.Y, dst.U, dst.V), want):
            assert np.array_equal(host(g[f:f + 1]), w_), ("output frame", f)
    return len(frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deband.json"))
    ap.add_argument("--frames", type=int, default=1024)
    args = ap.parse_args()
    import numpy as np
    import torch
    import amatsukaze_amd as A
    import deband_ref as R
    N = args.frames
    isa = kernel_isa()
    ctx = A.Context(0)
    ctx.profile(True)
    res = {"what": "Debander %dx%d, radius %d, threshold %d, sample %d, blur_first, %d frames in HBM, one launch per call, beside kfm_render_kernel with an "
                   "all-30p plan on the same buffers' sizes (a whole-frame copy); HIP events around the launches, median [min - max] of %d after %d "
                   "warm-up calls, the two alternating in the same run (tools/deband_bench.py).  The LDS figures are the guide's bank model on the "
                   "timed table, no counter was read: not measured.  The global-gather alternative was not built: not measured"
                   % (W, H, RADIUS, THRESHOLD, SAMPLE, N, REPS, WARMUP),
           "device": torch.cuda.get_device_name(0), "peak_TB_per_s": 8.0, "tile": [TW, TH], "isa": isa, "cases": []}
    plan = A.kfm_render_plan([2] * N, [0] * N)
    assert len(plan) == N
    for bits in (8, 14):
        es = 1 if bits <= 8 else 2
        frame = (W * H * 3 // 2) * es
        src = clip(A, torch, N, W, H, bits, seed=61 + bits)
        dst = clip(A, torch, N, W, H, bits)
        copy_dst = clip(A, torch, N, W, H, bits)
        db = A.Debander(ctx, (W, H), bits, RADIUS, THRESHOLD, SAMPLE, BLUR_FIRST, SEED)
        db.run(src, dst)
        checked = check_frames(np, R, src, dst, bits)
        ms = {"deband": [], "copy": []}
        for i in range(WARMUP + REPS):
            t = kernel_ms(ctx, "deband_kernel", lambda: db.run(src, dst))
            c = kernel_ms(ctx, "kfm_render_kernel", lambda: A.kfm_render(ctx, src, plan, copy_dst))
            if i >= WARMUP:
                ms["deband"].append(t); ms["copy"].append(c)
        sp = {k: spread(v) for k, v in ms.items()}
        form = isa[f"{8 * es}-bit containers, 16-byte lanes"]
        model = work_model(np, R, es)
        alg = 2.0 * N * frame
        requested = float(N) * (model["staged_bytes"] + model["table_bytes"] + frame)
        issue_ms = N * model["wave_steps"] * form["row_loop_vector_instructions"] * CYCLES_PER_WAVE_VALU / (CUS * SIMDS_PER_CU * CLOCK_HZ) * 1e3
        lds_cycles = model["reference_read_cycles"] + model["centre_read_cycles"] + model["staging_store_cycles"]
        lds_ms = N * lds_cycles / (CUS * CLOCK_HZ) * 1e3
        mem_ms = alg / HBM_PEAK * 1e3
        bounds = {"issue rate": issue_ms, "LDS reads": lds_ms, "bytes": mem_ms}
        px = 16 // es
        case = {"bits": bits, "frames": N, "frames_checked_against_numpy": checked, "ms": sp,
                "algorithmic_bytes": alg, "algorithmic": rates(alg, sp["deband"]),
                "requested_bytes": requested, "read_amplification_of_the_halo": model["staged_bytes"] / frame,
                "table_bytes_per_frame": model["table_bytes"],
                "vector_instructions_per_pixel": form["row_loop_vector_instructions"] / px,
                "wave_steps_per_frame": model["wave_steps"],
                "lds_cycles_per_frame": {k: model[k] for k in ("reference_read_cycles", "centre_read_cycles", "staging_store_cycles")},
                "lds_cycles_per_reference_read": model["reference_read_cycles"] / (model["wave_steps"] * 4 * px),
                "issue_rate_bound_ms": issue_ms, "lds_bound_ms_model": lds_ms, "memory_bound_ms_at_8TBps_algorithmic": mem_ms,
                "largest_bound": max(bounds, key=bounds.get),
                "measured_over_issue_rate_bound": sp["deband"]["median"] / issue_ms,
                "measured_over_lds_bound_model": sp["deband"]["median"] / lds_ms,
                "measured_over_memory_bound": sp["deband"]["median"] / mem_ms,
                "copy": {"bytes": alg, **rates(alg, sp["copy"])},
                "ratio_to_copy": sp["deband"]["median"] / sp["copy"]["median"]}
        res["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        db.close()
        del src, dst, copy_dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
