"""The deband on decoder surfaces (Debander.run with NV12 / P010 descriptors, csrc/deband_surface_kernels.hip) measured on an MI355X;
writes profiles/deband_surfaces.json.  Reported, not gated.

  1920x1080, 1 024 frames resident in HBM, radius 25, threshold 1, sample 2, blur_first (the server's KDeband(25, 1, 2, true)), one
  launch per call; NV12 (8-bit) and P010 (10 bits in the high bits of 16-bit containers, RANDOM low bits), random samples: the kernel's
  work does not depend on them (selects, no branches).  Times are the context's HIP events around the kernel launches of a call
  (Context.profile), median [min - max] of 7 after 2 warm-up calls.  Three routes to the same pictures, timed alternating in the same run:

    (a) surfaces   the in-kind filter: surfaces in, surfaces out (deband_surface_kernel);
    (b) planar     the planar kernel (deband_kernel) on a planar LSB copy of the same pictures -- the same rule on the same samples, the
                   yardstick for what the interleaved walk and the shifts cost;
    (c) planarise  the only route from surfaces before: weave_fields(nv12=True[, msb=True]) of ALL frames into planar LSB frames
                   (weave_fields_kernel), then (b).  Its time is the sum of the two kernels; it ENDS IN PLANAR FRAMES and holds a second
                   copy of the clip.

  Before any figure is reported the three outputs are compared at the timed size: (a) >> s de-interleaved equals (b) equals (c) in every
  container (s = 6 for P010, 0 for NV12), every container of (a) has zero low bits, and frames 0, the middle one and the last of (a)
  equal the numpy restatement (tests/deband_surfaces_ref.py).  Beside the times, from hipcc's assembly: each new form's registers and LDS
  bytes, and for the 16-byte forms the vector instructions per pixel of the row loop the timed case runs (sample 2 with blur_first),
  counted as tools/deband_bench.py counts the planar forms'; an interleaved form holds that loop twice, for the luma plane's cell and for
  the UV plane's, whose horizontal step is 2 containers.

    python tools/deband_surfaces_bench.py [--out profiles/deband_surfaces.json] [--frames 1024] [--isa-only]
There is no CPU path: without a GPU this fails (but for --isa-only)."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kfm_render_bench import H, REPS, W, WARMUP, kernel_ms, spread  # noqa: E402
from resize_bench import blocks_of, valu  # noqa: E402
from surface_render_bench import planar, samples, surfaces  # noqa: E402

RADIUS, THRESHOLD, SAMPLE, BLUR_FIRST, SEED = 25, 1, 2, True, 0
# (file, kernel, <template arguments> as the symbol spells them, form, bytes per container)
FORMS = (("deband_kernels.hip", "deband_kernel", "IhLb1E", "planar LSB, 8-bit, 16-byte lanes", 1),
         ("deband_kernels.hip", "deband_kernel", "ItLb1E", "planar LSB, 16-bit, 16-byte lanes", 2),
         ("deband_surface_kernels.hip", "deband_surface_kernel", "IhLb1ELb0ELb1E", "interleaved, 8-bit (NV12), 16-byte lanes", 1),
         ("deband_surface_kernels.hip", "deband_surface_kernel", "IhLb0ELb0ELb1E", "interleaved, 8-bit (NV12), container by container", 1),
         ("deband_surface_kernels.hip", "deband_surface_kernel", "ItLb1ELb0ELb1E", "interleaved, 16-bit LSB, 16-byte lanes", 2),
         ("deband_surface_kernels.hip", "deband_surface_kernel", "ItLb0ELb0ELb1E", "interleaved, 16-bit LSB, container by container", 2),
         ("deband_surface_kernels.hip", "deband_surface_kernel", "ItLb1ELb1ELb1E", "interleaved, 16-bit MSB (P010), 16-byte lanes", 2),
         ("deband_surface_kernels.hip", "deband_surface_kernel", "ItLb0ELb1ELb1E", "interleaved, 16-bit MSB (P010), container by container", 2),
         ("deband_surface_kernels.hip", "deband_surface_kernel", "ItLb1ELb1ELb0E", "planar, 16-bit MSB, 16-byte lanes", 2),
         ("deband_surface_kernels.hip", "deband_surface_kernel", "ItLb0ELb1ELb0E", "planar, 16-bit MSB, container by container", 2))


def kernel_isa():
    """{form: VGPRs, LDS bytes and, for the 16-byte forms, the vector instructions of the row loop(s) of sample 2 with blur_first, per
    lane step and per pixel}, the files compiled as build.py compiles them"""
    from test_isa_guards import kernels_of
    from test_isa_surfaces import compile_file
    asms, res = {}, {}
    for name, kernel, tag, form, es in FORMS:
        if name not in asms:
            asm = compile_file(name)
            lds = {re.search(r"\.name:\s+(\S+)", m.group(0)).group(1): int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", m.group(0)).group(1))
                   for m in re.finditer(r"- \.agpr_count:.*?\n(?=  - \.agpr_count:|\.\.\.|amdhsa\.target)", asm, re.S)}
            asms[name] = (kernels_of(asm), lds)
        ks, lds = asms[name]
        (sym,) = [n for n in ks if kernel + tag + "EEvNS" in n]
        res[form] = {"vgprs": ks[sym]["meta"]["vgpr_count"], "lds_bytes": lds[sym]}
        if "16-byte lanes" in form:
            px, read = 16 // es, "ds_read_u8" if es == 1 else "ds_read_u16"
            body = [l.strip() for l in ks[sym]["body"]]
            # the row loops of sample 2 hold four references per pixel; blur_first's is the one without the per-reference comparisons
            loops = sorted((b for b in blocks_of(body) if sum(l.startswith(read) for l in b) == 4 * px), key=valu)
            cells = 2 if "interleaved" in form else 1
            assert len(loops) == 2 * cells, (sym, len(loops))
            timed = [valu(b) for b in loops[:cells]]
            res[form].update({"pixels_per_lane_step": px, "row_loop_vector_instructions": timed,
                              "vector_instructions_per_pixel": [v / px for v in timed],
                              "row_loop_packed_16_bit_shifts": [sum(l.startswith("v_pk_lsh") for l in b) for b in loops[:cells]],
                              "row_loop_full_width_multiplies": sum(l.startswith("v_mul_lo_u32") for b in loops for l in b)})
    return res


def routes_equal(torch, s, out_a, out_b, out_c):
    """the contract of DESIGN.md section 6f at the timed size, frame by frame (no whole-clip temporaries)"""
    low = (1 << s) - 1
    for k in range(out_a.num_frames):
        a = (samples(torch, out_a.Y[k], s), samples(torch, out_a.U[k, :, 0::2], s), samples(torch, out_a.U[k, :, 1::2], s))
        for x, pb, pc in zip(a, (out_b.Y[k], out_b.U[k], out_b.V[k]), (out_c.Y[k], out_c.U[k], out_c.V[k])):
            if not (torch.equal(x, samples(torch, pb, 0)) and torch.equal(pb, pc)):
                return False
        if low and any(bool(((P[k].to(torch.int32) & low) != 0).any()) for P in (out_a.Y, out_a.U)):
            return False
    return True


def check_frames(np, DS, src, out_a, bits, msb):
    dt = np.uint8 if bits <= 8 else np.uint16
    host = lambda t: t.cpu().numpy().view(dt)
    n = src.num_frames
    frames = sorted({0, n // 2, n - 1})
    for f in frames:
        want = DS.deband_surfaces((host(src.Y[f:f + 1]), host(src.U[f:f + 1])), bits, True, msb, RADIUS, THRESHOLD, SAMPLE, BLUR_FIRST, SEED)
        for g, w_ in zip((out_a.Y, out_a.U), want):
            assert np.array_equal(host(g[f:f + 1]), w_), ("output frame", f)
    return len(frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deband_surfaces.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--isa-only", action="store_true", help="print the registers and instruction counts and stop (needs no GPU)")
    args = ap.parse_args()
    isa = kernel_isa()
    if args.isa_only:
        print(json.dumps(isa, indent=1))
        return
    import numpy as np
    import torch
    import amatsukaze_amd as A
    import deband_surfaces_ref as DS
    N = args.frames
    ctx = A.Context(0)
    ctx.profile(True)
    res = {"what": "Debander on decoder surfaces, %dx%d, %d frames in HBM, radius %d, threshold %d, sample %d, blur_first, one launch per call; HIP "
                   "events around the launches, median [min - max] of %d after %d warm-up calls (tools/deband_surfaces_bench.py); routes: surfaces = "
                   "in kind, planar = the planar kernel on a planar LSB copy, planarise = weave_fields of every frame + the planar kernel (ends in "
                   "planar frames, holds a second copy of the clip)" % (W, H, N, RADIUS, THRESHOLD, SAMPLE, REPS, WARMUP),
           "device": torch.cuda.get_device_name(0), "isa": isa, "cases": []}
    for layout, bits, msb in (("NV12", 8, False), ("P010", 10, True)):
        s = 16 - bits if msb else 0
        src = surfaces(A, torch, N, bits, msb, seed=71 + bits)
        src_planar = planar(A, torch, N, bits)                        # (b) reads it; (c) rewrites it with the same samples on every call

        def planarise():
            A.weave_fields(ctx, src.Y, src.U, None, src_planar, nv12=True, msb=msb)
            ctx.synchronize()

        planarise()
        out_a, out_b, out_c = surfaces(A, torch, N, bits, msb), planar(A, torch, N, bits), planar(A, torch, N, bits)
        db = A.Debander(ctx, (W, H), bits, RADIUS, THRESHOLD, SAMPLE, BLUR_FIRST, SEED)
        run_a, run_b, run_c = (lambda: db.run(src, out_a)), (lambda: db.run(src_planar, out_b)), (lambda: db.run(src_planar, out_c))
        run_a(); run_b(); planarise(); run_c()
        equal = routes_equal(torch, s, out_a, out_b, out_c)
        checked = check_frames(np, DS, src, out_a, bits, msb)
        ms = {"surfaces": [], "planar": [], "planarise": []}
        for i in range(WARMUP + REPS):
            ta = kernel_ms(ctx, "deband_surface_kernel", run_a)
            tb = kernel_ms(ctx, "deband_kernel", run_b)
            tc = kernel_ms(ctx, "weave_fields_kernel", planarise) + kernel_ms(ctx, "deband_kernel", run_c)
            if i >= WARMUP:
                ms["surfaces"].append(ta); ms["planar"].append(tb); ms["planarise"].append(tc)
        t = {k: spread(v) for k, v in ms.items()}
        apart = lambda x, y: bool(x["max"] < y["min"] or y["max"] < x["min"])
        d = t["surfaces"]["median"] - t["planar"]["median"]
        case = {"layout": layout, "bits": bits, "frames": N, "outputs_of_the_three_routes_equal": bool(equal), "frames_checked_against_numpy": checked,
                "surfaces": {"ms": t["surfaces"]}, "planar": {"ms": t["planar"]},
                "planarise_then_planar": {"ms": t["planarise"], "ends_in": "planar frames"},
                "surfaces_minus_planar_ms": d, "surfaces_minus_planar_share": d / t["planar"]["median"],
                "surfaces_vs_planar_ranges_apart": apart(t["surfaces"], t["planar"]),
                "planarise_over_surfaces": t["planarise"]["median"] / t["surfaces"]["median"],
                "surfaces_under_planarise_ranges_apart": bool(t["surfaces"]["max"] < t["planarise"]["min"])}
        print(json.dumps(case), file=sys.stderr, flush=True)
        assert equal, "the three routes differ"                       # nothing is reported of such a run
        res["cases"].append(case)
        db.close()
        del src, src_planar, out_a, out_b, out_c
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
