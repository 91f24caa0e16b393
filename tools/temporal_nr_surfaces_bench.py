"""The temporal noise reduction on decoder surfaces (temporal_nr with NV12 / P010 descriptors, csrc/temporal_nr_surface_kernels.hip)
measured on an MI355X; writes profiles/temporal_nr_surfaces.json.  Reported, not gated.

  1920x1080, 1 024 frames resident in HBM, temporal_distance 3, threshold 1 (the server's KTemporalNR(3, 1)), NV12 (8-bit) and P010 (10
  bits in the high bits of 16-bit containers, RANDOM low bits).  The clip is a still random picture with per-frame noise of 0 .. 2 on
  every sample, so that windows do pass frames; the kernel's work does not depend on the samples (a select, not a branch).  Times are
  the context's HIP events around the kernel launches of a call (Context.profile), median [min - max] of 7 after 2 warm-up calls.  Three
  routes to the same pictures, timed alternating in the same run:

    (a) surfaces   the in-kind filter: surfaces in, surfaces out (temporal_nr_surfaces_kernel);
    (b) planar     the planar kernel (temporal_nr_kernel) on a planar LSB copy of the same pictures -- the same rule on the same samples,
                   the yardstick for what the de-interleave and the shifts cost;
    (c) planarise  the only route from surfaces before: weave_fields(nv12=True[, msb=True]) of ALL frames into planar LSB frames
                   (weave_fields_kernel), then (b).  Its time is the sum of the two kernels; it ENDS IN PLANAR FRAMES and holds a second
                   copy of the clip.

  Before any figure is reported the three outputs are compared at the timed size: (a) >> s de-interleaved equals (b) equals (c) in every
  container (s = 6 for P010, 0 for NV12), every container of (a) has zero low bits, and the filter changed more than 5 % of the samples
  of a middle frame.  Beside the times, from hipcc's assembly: each form's registers, and the vector instructions per luma pixel of the
  16-byte forms' two window loops (the planar kernel's are 145 at 8 bits and 146 at 16).

    python tools/temporal_nr_surfaces_bench.py [--out profiles/temporal_nr_surfaces.json] [--frames 1024] [--isa-only]
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
from surface_render_bench import planar, samples, surfaces  # noqa: E402

D, THRESHOLD = 3, 1
# (file, kernel, <template arguments> as the symbol spells them, form, bytes per container)
FORMS = (("temporal_nr_kernels.hip", "temporal_nr_kernel", "IhLb1E", "planar LSB, 8-bit, 16-byte lanes", 1),
         ("temporal_nr_kernels.hip", "temporal_nr_kernel", "ItLb1E", "planar LSB, 16-bit, 16-byte lanes", 2),
         ("temporal_nr_surface_kernels.hip", "temporal_nr_surfaces_kernel", "IhLb1ELb0ELb1E", "interleaved, 8-bit (NV12), 16-byte lanes", 1),
         ("temporal_nr_surface_kernels.hip", "temporal_nr_surfaces_kernel", "IhLb0ELb0ELb1E", "interleaved, 8-bit (NV12), container by container", 1),
         ("temporal_nr_surface_kernels.hip", "temporal_nr_surfaces_kernel", "ItLb1ELb0ELb1E", "interleaved, 16-bit LSB, 16-byte lanes", 2),
         ("temporal_nr_surface_kernels.hip", "temporal_nr_surfaces_kernel", "ItLb0ELb0ELb1E", "interleaved, 16-bit LSB, container by container", 2),
         ("temporal_nr_surface_kernels.hip", "temporal_nr_surfaces_kernel", "ItLb1ELb1ELb1E", "interleaved, 16-bit MSB (P010), 16-byte lanes", 2),
         ("temporal_nr_surface_kernels.hip", "temporal_nr_surfaces_kernel", "ItLb0ELb1ELb1E", "interleaved, 16-bit MSB (P010), container by container", 2),
         ("temporal_nr_surface_kernels.hip", "temporal_nr_surfaces_kernel", "ItLb1ELb1ELb0E", "planar, 16-bit MSB, 16-byte lanes", 2),
         ("temporal_nr_surface_kernels.hip", "temporal_nr_surfaces_kernel", "ItLb0ELb1ELb0E", "planar, 16-bit MSB, container by container", 2))


def kernel_isa():
    """{form: VGPRs, and for the 16-byte forms the vector instructions of the count loop and of the sum loop and, from them, per luma
    pixel at temporal_distance 3}, the files compiled as build.py compiles them"""
    from test_isa_guards import kernels_of
    from test_isa_surfaces import compile_file
    asms, res = {}, {}
    for name, kernel, tag, form, es in FORMS:
        if name not in asms:
            asms[name] = compile_file(name)
        asm = asms[name]
        (sym,) = [n for n in kernels_of(asm) if kernel + tag + "E" in n]
        res[form] = {"vgprs": kernels_of(asm)[sym]["meta"]["vgpr_count"]}
        if "16-byte lanes" in form:
            text = asm[asm.index("\n" + sym + ":"):]
            loops = re.findall(r"^(\.LBB\d+_\d+):[^\n]*Inner Loop Header[^\n]*\n(.*?)^\s+s_cbranch_\w+ \1$", text, re.M | re.S)[:2]
            assert len(loops) == 2, (sym, len(loops))
            valu = [sum(bool(re.match(r"\s+v_", l)) for l in body.split("\n")) for _, body in loops]
            res[form].update({"count_loop_vector_instructions": valu[0], "sum_loop_vector_instructions": valu[1],
                              "vector_instructions_per_luma_pixel": (valu[0] + valu[1]) * (2 * D + 1) / (2 * (16 // es))})
    return res


def noisy_surfaces(A, torch, n, bits, msb, seed):
    """NV12-layout surfaces of a still random picture (away from the range's ends) with noise of 0 .. 2 on every sample of every frame;
    MSB: sample << s with random low bits"""
    s = 16 - bits if msb else 0
    out = surfaces(A, torch, n, bits, msb)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    for P in (out.Y, out.U):
        still = torch.randint(1, (1 << bits) - 3, (1,) + tuple(P.shape[1:]), dtype=torch.int32, device="cuda", generator=gen)
        for f in range(n):                                            # (frame by frame: no whole-clip temporaries)
            v = (still[0] + torch.randint(0, 3, tuple(P.shape[1:]), dtype=torch.int32, device="cuda", generator=gen)) << s
            if s:
                v |= torch.randint(0, 1 << s, tuple(P.shape[1:]), dtype=torch.int32, device="cuda", generator=gen)
            P[f] = (v if bits <= 8 else torch.where(v >= 32768, v - 65536, v)).to(P.dtype)
    return out


def routes_equal(torch, s, src, out_a, out_b, out_c):
    """(the identity of DESIGN.md section 9 at the timed size, the share of a middle frame's luma samples that the filter changed)"""
    low = (1 << s) - 1
    for k in range(out_a.num_frames):
        a = (samples(torch, out_a.Y[k], s), samples(torch, out_a.U[k, :, 0::2], s), samples(torch, out_a.U[k, :, 1::2], s))
        for x, pb, pc in zip(a, (out_b.Y[k], out_b.U[k], out_b.V[k]), (out_c.Y[k], out_c.U[k], out_c.V[k])):
            if not (torch.equal(x, samples(torch, pb, 0)) and torch.equal(pb, pc)):
                return False, 0.0
        if low and any(bool(((P[k].to(torch.int32) & low) != 0).any()) for P in (out_a.Y, out_a.U)):
            return False, 0.0
    k = out_a.num_frames // 2
    changed = float((samples(torch, out_a.Y[k], s) != samples(torch, src.Y[k], s)).float().mean())
    return True, changed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_nr_surfaces.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--isa-only", action="store_true", help="print the registers and instruction counts and stop (needs no GPU)")
    args = ap.parse_args()
    isa = kernel_isa()
    if args.isa_only:
        print(json.dumps(isa, indent=1))
        return
    import torch
    import amatsukaze_amd as A
    N = args.frames
    ctx = A.Context(0)
    ctx.profile(True)
    res = {"what": "temporal_nr on decoder surfaces, %dx%d, %d frames in HBM, temporal_distance %d, threshold %d; HIP events around the launches, "
                   "median [min - max] of %d after %d warm-up calls (tools/temporal_nr_surfaces_bench.py); routes: surfaces = in kind, planar = the "
                   "planar kernel on a planar LSB copy, planarise = weave_fields of every frame + the planar kernel (ends in planar frames, holds "
                   "a second copy of the clip)" % (W, H, N, D, THRESHOLD, REPS, WARMUP),
           "device": torch.cuda.get_device_name(0), "isa": isa, "cases": []}
    for layout, bits, msb in (("NV12", 8, False), ("P010", 10, True)):
        s = 16 - bits if msb else 0
        src = noisy_surfaces(A, torch, N, bits, msb, seed=57 + bits)
        src_planar = planar(A, torch, N, bits)                        # (b) reads it; (c) rewrites it with the same samples on every call

        def planarise():
            A.weave_fields(ctx, src.Y, src.U, None, src_planar, nv12=True, msb=msb)
            ctx.synchronize()

        planarise()
        out_a, out_b, out_c = surfaces(A, torch, N, bits, msb), planar(A, torch, N, bits), planar(A, torch, N, bits)
        run_a = lambda: A.temporal_nr(ctx, src, out_a, D, THRESHOLD)
        run_b = lambda: A.temporal_nr(ctx, src_planar, out_b, D, THRESHOLD)
        run_c = lambda: A.temporal_nr(ctx, src_planar, out_c, D, THRESHOLD)
        run_a(); run_b(); planarise(); run_c()
        equal, changed = routes_equal(torch, s, src, out_a, out_b, out_c)
        ms = {"surfaces": [], "planar": [], "planarise": []}
        for i in range(WARMUP + REPS):
            ta = kernel_ms(ctx, "temporal_nr_surfaces_kernel", run_a)
            tb = kernel_ms(ctx, "temporal_nr_kernel", run_b)
            tc = kernel_ms(ctx, "weave_fields_kernel", planarise) + kernel_ms(ctx, "temporal_nr_kernel", run_c)
            if i >= WARMUP:
                ms["surfaces"].append(ta); ms["planar"].append(tb); ms["planarise"].append(tc)
        t = {k: spread(v) for k, v in ms.items()}
        d = t["surfaces"]["median"] - t["planar"]["median"]
        case = {"layout": layout, "bits": bits, "frames": N, "outputs_of_the_three_routes_equal": bool(equal),
                "luma_samples_of_a_middle_frame_changed": changed,
                "surfaces": {"ms": t["surfaces"]}, "planar": {"ms": t["planar"]},
                "planarise_then_planar": {"ms": t["planarise"], "ends_in": "planar frames"},
                "surfaces_minus_planar_ms": d, "surfaces_minus_planar_share": d / t["planar"]["median"],
                "surfaces_outside_planar_spread": bool(not t["planar"]["min"] <= t["surfaces"]["median"] <= t["planar"]["max"]),
                "planarise_over_surfaces": t["planarise"]["median"] / t["surfaces"]["median"]}
        print(json.dumps(case), file=sys.stderr, flush=True)
        assert equal and changed > 0.05, "the three routes differ, or the filter had nothing to do"      # nothing is reported of such a run
        res["cases"].append(case)
        del src, src_planar, out_a, out_b, out_c
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
