"""The edge level (edge_level, csrc/edgelevel_kernels.hip) measured on an MI355X beside a whole-frame copy; writes profiles/edgelevel.json.

  1920x1080 at 8 and at 14 bits, 1 024 frames resident in HBM, strength 16, threshold 10, repair 2 (the server's KEdgeLevel(16, 10, 2)),
  one launch per call, on the soft content of tests/edgelevel_ref.py (a 240 x 136 clip of 8 frames) tiled to size.  The comparator is
  kfm_render with an all-30p plan on the same source and a buffer of the destination's size -- a whole-frame copy -- alternating with
  the edge level in the same run.  Times are the context's HIP events around the kernel launch of a call (Context.profile), median
  [min - max] of 7 after 2 warm-up calls.

  Bytes: algorithmic = the source read once plus the destination written once, which is also the copy's.  The kernel requests the four
  halo rows of every strip of 32 a second time: 1.125 x the luma reads (caches may serve them: not measured).

  From the ISA (the file compiled as build.py compiles it), for the 16-byte form the timed case runs: the vector instructions of the
  row loop of repair 2 per lane and output row (16 bytes), the blocks only the lane with a row's last containers runs left out, and
  the bound they give -- wave-instructions x 2 cycles (a SIMD of 32 lanes issues a wave's instruction in 2, with at least two waves
  to a SIMD) over 256 CUs x 4 SIMDs at 2.4 GHz, idle lanes of partly filled waves counted as issued, the scalar unit not counted --
  beside the bytes' bound at 8 TB/s.  No counter was read: what limits the kernel beyond these two figures is not measured.
  The LDS-tile alternative was not built: not measured.

  Before any timing the call's output on the 240 x 136 clip is compared with the numpy restatement (tests/edgelevel_ref.py) in full,
  and output frames 0, the middle one and the last of the timed clip as well.

    python tools/edgelevel_bench.py [--out profiles/edgelevel.json] [--frames 1024]
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
from resize_bench import clip  # noqa: E402

PARAMS = (16, 10, 2)
STRIP, SPAN_BYTES = 32, 64 * 16                  # kEdgeStripRows, kEdgeSpanBytes (csrc/kernels.hpp)
TILE_W, TILE_H, TILE_N = 240, 136, 8
CUS, SIMDS_PER_CU, CLOCK_HZ, CYCLES_PER_WAVE_VALU = 256, 4, 2.4e9, 2
NARROW = re.compile(r"global_(load_ubyte|load_ushort|load_sbyte|store_byte|store_short)")


def row_loops(body):
    """the innermost loops that hold the cell (its 24-bit multiplies): [(vector instructions all lanes run, instructions, multiplies)],
    one per repair.  A loop is the blocks from a backward branch's target to the branch; blocks with container-wide accesses are the
    tail lane's"""
    lines = [l.strip() for l in body]
    label_at = {l[:-1]: i for i, l in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:$", l)}
    spans = []
    for i, l in enumerate(lines):
        m = re.match(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)$", l) or re.match(r"s_branch\s+(\.LBB\d+_\d+)$", l)
        if m and label_at.get(m.group(1), i) < i:
            spans.append((label_at[m.group(1)], i))
    out = []
    for a, b in spans:
        seg = lines[a:b + 1]
        muls = sum(x.startswith("v_mul_i32_i24") for x in seg)
        if not muls or any(a <= a2 and b2 <= b and (a2, b2) != (a, b) and any(x.startswith("v_mul_i32_i24") for x in lines[a2:b2 + 1]) for a2, b2 in spans):
            continue                                 # no cell, or an outer loop around one
        blocks, cur = [], []
        for x in seg:
            if x.endswith(":"):
                blocks.append(cur)
                cur = []
            else:
                cur.append(x)
        blocks.append(cur)
        common = [x for blk in blocks if not any(NARROW.match(y) for y in blk) for x in blk]
        out.append((sum(x.startswith("v_") for x in common), len(common), muls))
    return out


def kernel_isa():
    """{form: registers and the instructions of the row loop the timed case runs} for the two 16-byte forms"""
    from test_isa_guards import kernels_of
    from test_isa_surfaces import compile_file
    res = {}
    for name, k in kernels_of(compile_file("edgelevel_kernels.hip")).items():
        for t, es in (("h", 1), ("t", 2)):
            if f"edgelevel_kernelI{t}Lb1E" not in name:
                continue
            loops = sorted(row_loops(k["body"]))
            assert len(loops) == 5, (name, loops)                                                  # repair 0..4: each adds to the one before
            v, n, _ = loops[PARAMS[2]]
            res[f"{8 * es}-bit containers, 16-byte lanes"] = {
                "vgprs": k["meta"]["vgpr_count"], "pixels_per_lane_row": 16 // es, "row_loop_vector_instructions": v, "row_loop_instructions": n,
                "row_loop_vector_instructions_by_repair": [x for x, _, _ in loops]}
    return res


def soft_clip(np, torch, A, R, n, bits):
    """the 240 x 136 soft clip tiled to W x H and n frames, on the device; chroma uniform random"""
    tile = R.clip(TILE_W, TILE_H, (bits, bits), "soft", TILE_N)
    dt = torch.uint8 if bits <= 8 else torch.int16
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8 if bits <= 8 else np.int16)).cuda()
    Y = dev(tile[0]).repeat(-(-n // TILE_N), -(-H // TILE_H), -(-W // TILE_W))[:n, :H, :W].contiguous()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(71 + bits)
    U, V = (torch.randint(0, 1 << bits, (n, H // 2, W // 2), dtype=dt, device="cuda", generator=gen) for _ in range(2))
    return A.DeviceClip(Y, U, V, W, H, bits)


def check_small(np, torch, A, R, ctx, bits):
    """the whole call on the tile clip against the restatement"""
    dt = np.uint8 if bits <= 8 else np.uint16
    planes = R.clip(TILE_W, TILE_H, (bits, bits), "soft", TILE_N)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8 if bits <= 8 else np.int16)).cuda()
    src = A.DeviceClip(*(dev(p) for p in planes), TILE_W, TILE_H, bits)
    dst = clip(A, torch, TILE_N, TILE_W, TILE_H, bits)
    assert A.edge_level(ctx, src, dst, *PARAMS) == TILE_N
    want = R.filter_clip(planes, bits, *PARAMS)
    for g, w_ in zip((dst.Y, dst.U, dst.V), want):
        assert np.array_equal(g.cpu().numpy().view(dt), w_), "the reduced clip differs from the restatement"
    return float(np.mean(want[0] != planes[0]))


def check_frames(np, R, src, dst, bits):
    dt = np.uint8 if bits <= 8 else np.uint16
    host = lambda t: t.cpu().numpy().view(dt)
    n = src.num_frames
    frames = sorted({0, n // 2, n - 1})
    for f in frames:
        want = R.filter_clip(tuple(host(p[f:f + 1]) for p in (src.Y, src.U, src.V)), bits, *PARAMS)
        for g, w_ in zip((dst.Y, dst.U, dst.V), want):
            assert np.array_equal(host(g[f:f + 1]), w_), ("output frame", f)
    return len(frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edgelevel.json"))
    ap.add_argument("--frames", type=int, default=1024)
    args = ap.parse_args()
    import numpy as np
    import torch
    import amatsukaze_amd as A
    import edgelevel_ref as R
    N = args.frames
    isa = kernel_isa()
    ctx = A.Context(0)
    ctx.profile(True)
    res = {"what": "edge_level %dx%d, strength %d, threshold %d, repair %d, %d frames in HBM of the soft content tiled to size, one launch per call, "
                   "beside kfm_render_kernel with an all-30p plan on the same buffers' sizes (a whole-frame copy); HIP events around the launches, "
                   "median [min - max] of %d after %d warm-up calls, the two alternating in the same run (tools/edgelevel_bench.py).  The issue-rate "
                   "bound is counted from the ISA; no counter was read: what limits the kernel beyond the two bounds is not measured.  The LDS-tile "
                   "alternative was not built: not measured" % ((W, H) + PARAMS + (N, REPS, WARMUP)),
           "device": torch.cuda.get_device_name(0), "peak_TB_per_s": 8.0, "strip_rows": STRIP, "span_bytes": SPAN_BYTES, "isa": isa, "cases": []}
    plan = A.kfm_render_plan([2] * N, [0] * N)
    assert len(plan) == N
    for bits in (8, 14):
        es = 1 if bits <= 8 else 2
        frame = (W * H * 3 // 2) * es
        changed_small = check_small(np, torch, A, R, ctx, bits)
        src = soft_clip(np, torch, A, R, N, bits)
        dst = clip(A, torch, N, W, H, bits)
        copy_dst = clip(A, torch, N, W, H, bits)
        A.edge_level(ctx, src, dst, *PARAMS)
        checked = check_frames(np, R, src, dst, bits)
        ms = {"edgelevel": [], "copy": []}
        for i in range(WARMUP + REPS):
            t = kernel_ms(ctx, "edgelevel_kernel", lambda: A.edge_level(ctx, src, dst, *PARAMS))
            c = kernel_ms(ctx, "kfm_render_kernel", lambda: A.kfm_render(ctx, src, plan, copy_dst))
            if i >= WARMUP:
                ms["edgelevel"].append(t); ms["copy"].append(c)
        sp = {k: spread(v) for k, v in ms.items()}
        form = isa[f"{8 * es}-bit containers, 16-byte lanes"]
        spans, strips = -(-W * es // SPAN_BYTES), -(-H // STRIP)
        # a wave runs its row loop once per row of its strip and per halo row: rows + 4 iterations, whole waves
        wave_rows = spans * (H + 4 * strips)
        alg = 2.0 * N * frame
        issue_ms = N * wave_rows * form["row_loop_vector_instructions"] * CYCLES_PER_WAVE_VALU / (CUS * SIMDS_PER_CU * CLOCK_HZ) * 1e3
        mem_ms = alg / HBM_PEAK * 1e3
        bounds = {"issue rate": issue_ms, "bytes": mem_ms}
        larger = max(bounds.values())
        case = {"bits": bits, "frames": N, "frames_checked_against_numpy": checked, "share_of_luma_changed_on_the_reduced_clip": changed_small, "ms": sp,
                "algorithmic_bytes": alg, "algorithmic": rates(alg, sp["edgelevel"]),
                "requested_luma_read_amplification": (H + 4.0 * strips) / H,
                "vector_instructions_per_pixel": form["row_loop_vector_instructions"] / (16 // es),
                "wave_row_iterations_per_frame": wave_rows,
                "issue_rate_bound_ms": issue_ms, "memory_bound_ms_at_8TBps_algorithmic": mem_ms, "largest_bound": max(bounds, key=bounds.get),
                "measured_over_issue_rate_bound": sp["edgelevel"]["median"] / issue_ms, "measured_over_memory_bound": sp["edgelevel"]["median"] / mem_ms,
                "measured_above_the_larger_bound_ms": sp["edgelevel"]["median"] - larger, "copy_spread_ms": sp["copy"]["max"] - sp["copy"]["min"],
                "copy": {"bytes": alg, **rates(alg, sp["copy"])},
                "ratio_to_copy": sp["edgelevel"]["median"] / sp["copy"]["median"]}
        res["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        del src, dst, copy_dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
