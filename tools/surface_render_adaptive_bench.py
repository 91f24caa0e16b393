"""The adaptive bob on decoder surfaces (kfm_render(..., deint="adaptive") with NV12 / P010 descriptors,
csrc/render_adaptive_surface_kernels.hip) measured on an MI355X; writes profiles/surface_render_adaptive.json.  Reported, not gated.

  1920x1080, 1 024 source frames resident in HBM, NV12 (8-bit) and P010 (10 bits in the high bits of 16-bit containers, RANDOM low bits),
  the all-60i plan (every output frame a bob).  Times are the context's HIP events around the kernel launches of a call
  (Context.profile), median [min - max] of 7 after 2 warm-up calls.  Three routes to the same pictures, timed alternating in the same run:

    (a) surfaces   the in-kind adaptive render: surfaces in, surfaces out (kfm_render_adaptive_surfaces_kernel);
    (b) planar     the planar adaptive kernel (kfm_render_adaptive_kernel) on a planar LSB copy of the same pictures -- the same rule on
                   the same samples, the yardstick for what the step-2 neighbours of an interleaved row and the shifts cost;
    (c) planarise  the only route from surfaces before: weave_fields(nv12=True[, msb=True]) of ALL source frames into planar LSB frames
                   (weave_fields_kernel), then (b).  Its time is the sum of the two kernels; it ENDS IN PLANAR FRAMES.

  Before any figure is reported the three outputs are compared at the timed size: (a) >> s de-interleaved equals (b) equals (c) in every
  container (s = 6 for P010, 0 for NV12), and for P010 every interpolated row of (a) has zero low bits and every copied row is its source
  row.  Beside the times: the vector instructions per 16-byte span of each vector form's row functions, read from hipcc's assembly (the
  planar kernel's are 1 200 at 8 bits and 788 at 16).

    python tools/surface_render_adaptive_bench.py [--out profiles/surface_render_adaptive.json] [--frames 1024]
There is no CPU path: without a GPU this fails."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kfm_render_bench import H, REPS, W, WARMUP, kernel_ms, spread  # noqa: E402
from surface_render_bench import planar, routes_equal, surfaces  # noqa: E402

FORMS = (("render_adaptive_kernels.hip", "kfm_render_adaptive_kernel", "ILi1ELb1E", "planar LSB, 8-bit"),
         ("render_adaptive_kernels.hip", "kfm_render_adaptive_kernel", "ILi2ELb1E", "planar LSB, 16-bit"),
         ("render_adaptive_surface_kernels.hip", "kfm_render_adaptive_surfaces_kernel", "ILi1ELb1ELb0ELb1E", "interleaved, 8-bit (NV12)"),
         ("render_adaptive_surface_kernels.hip", "kfm_render_adaptive_surfaces_kernel", "ILi2ELb1ELb0ELb1E", "interleaved, 16-bit LSB"),
         ("render_adaptive_surface_kernels.hip", "kfm_render_adaptive_surfaces_kernel", "ILi2ELb1ELb1ELb1E", "interleaved, 16-bit MSB (P010)"),
         ("render_adaptive_surface_kernels.hip", "kfm_render_adaptive_surfaces_kernel", "ILi2ELb1ELb1ELb0E", "planar, 16-bit MSB"))


def span_loops_isa():
    """{form: {row function: vector instructions (and all instructions) in its loop that holds the 12 loads of a span}}, from hipcc's
    assembly.  An interleaved form has two such loops: the unit-step one of the luma rows and the step-2 one of the UV rows, told apart
    by their DPP moves (more dwords come from the neighbouring lanes at step 2)"""
    from amatsukaze_amd import build as B
    asms, res = {}, {}
    for name, kernel, tag, form in FORMS:
        if name not in asms:
            flags = [f for f in B.FLAGS if f != "-fPIC"] + B.EXTRA_FLAGS.get(name, [])
            with tempfile.TemporaryDirectory() as tmp:
                out = os.path.join(tmp, "k.s")
                subprocess.check_call([B.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(B.CSRC, name)], stderr=subprocess.DEVNULL)
                asms[name] = open(out).read()
        m = re.search(r"^(_ZN3amt\d+%s%sE\w*):[^\n]*\n(.*?)^\.Lfunc_end" % (kernel, tag), asms[name], re.M | re.S)
        blocks, cur = [], None                                        # (label, loop header or None, instructions)
        for line in m.group(2).split("\n"):
            b = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.(\d+):)\s*(?:;\s*(.*))?$", line)
            if b:
                note = b.group(3) or ""
                h = re.search(r"Header=(BB\d+_\d+)", note)
                cur = [b.group(1) or b.group(2), h.group(1) if h else (b.group(1) if "Loop Header" in note else None), []]
                blocks.append(cur)
            elif cur is not None and re.match(r"^\s+[a-z]", line):
                cur[2].append(line.strip())
        loops = {}
        for lbl, loop, ins in blocks:
            if loop is not None:
                loops.setdefault(loop, []).extend(ins)
        spans = [body for body in loops.values() if sum(i.startswith("global_load_dwordx4") for i in body) >= 12]
        spans.sort(key=lambda body: sum("_dpp" in i for i in body))
        names = ["unit step"] if len(spans) == 1 else ["unit step (luma rows)", "step 2 (UV rows)"]
        assert len(spans) == len(names), (form, len(spans))
        res[form] = {n: {"vector_instructions_per_span": sum(i.startswith("v_") for i in body), "instructions_per_span": len(body),
                         "packed_16_bit": sum(i.startswith("v_pk_") for i in body), "dpp_moves": sum("_dpp" in i for i in body),
                         "loads_16_bytes": sum(i.startswith("global_load_dwordx4") for i in body),
                         "container_loads_on_seam_lanes": sum(bool(re.match(r"global_load_(ubyte|ushort)", i)) for i in body)}
                     for n, body in zip(names, spans)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_render_adaptive.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--isa-only", action="store_true", help="print the instruction counts and stop (needs no GPU)")
    args = ap.parse_args()
    isa = span_loops_isa()
    if args.isa_only:
        print(json.dumps(isa, indent=1))
        return
    import torch
    import amatsukaze_amd as A
    N = args.frames
    ctx = A.Context(0)
    ctx.profile(True)
    res = {"what": "kfm_render(deint='adaptive') on decoder surfaces, %dx%d, %d source frames in HBM, all-60i plan; HIP events around the launches, "
                   "median [min - max] of %d after %d warm-up calls (tools/surface_render_adaptive_bench.py); routes: surfaces = in kind, planar = the "
                   "planar adaptive kernel on a planar LSB copy, planarise = weave_fields of every source frame + the planar adaptive kernel (ends in "
                   "planar frames)" % (W, H, N, REPS, WARMUP),
           "device": torch.cuda.get_device_name(0), "span_loops_from_the_isa": isa, "cases": []}
    plan = A.kfm_render_plan([0] * N, [0] * N)
    nout = len(plan)
    for layout, bits, msb in (("NV12", 8, False), ("P010", 10, True)):
        s = 16 - bits if msb else 0
        src = surfaces(A, torch, N, bits, msb, seed=91 + bits)
        src_planar = planar(A, torch, N, bits)                    # (b) reads it; (c) rewrites it with the same samples on every call

        def planarise():
            A.weave_fields(ctx, src.Y, src.U, None, src_planar, nv12=True, msb=msb)
            ctx.synchronize()

        planarise()
        out_a, out_b, out_c = surfaces(A, torch, nout, bits, msb), planar(A, torch, nout, bits), planar(A, torch, nout, bits)
        render_a = lambda: A.kfm_render(ctx, src, plan, out_a, deint="adaptive")
        render_b = lambda: A.kfm_render(ctx, src_planar, plan, out_b, deint="adaptive")
        render_c = lambda: A.kfm_render(ctx, src_planar, plan, out_c, deint="adaptive")
        render_a(); render_b(); planarise(); render_c()
        equal = routes_equal(torch, plan, s, src, out_a, out_b, out_c)
        ms = {"surfaces": [], "planar": [], "planarise": []}
        for i in range(WARMUP + REPS):
            ta = kernel_ms(ctx, "kfm_render_adaptive_surfaces_kernel", render_a)
            tb = kernel_ms(ctx, "kfm_render_adaptive_kernel", render_b)
            tc = kernel_ms(ctx, "weave_fields_kernel", planarise) + kernel_ms(ctx, "kfm_render_adaptive_kernel", render_c)
            if i >= WARMUP:
                ms["surfaces"].append(ta); ms["planar"].append(tb); ms["planarise"].append(tc)
        t = {k: spread(v) for k, v in ms.items()}
        d = t["surfaces"]["median"] - t["planar"]["median"]
        case = {"layout": layout, "bits": bits, "plan": "all-60i", "source_frames": N, "output_frames": nout,
                "outputs_of_the_three_routes_equal": bool(equal),
                "surfaces": {"ms": t["surfaces"]}, "planar": {"ms": t["planar"]},
                "planarise_then_planar": {"ms": t["planarise"], "ends_in": "planar frames"},
                "surfaces_minus_planar_ms": d, "surfaces_minus_planar_share": d / t["planar"]["median"],
                "surfaces_outside_planar_spread": bool(not t["planar"]["min"] <= t["surfaces"]["median"] <= t["planar"]["max"]),
                "planarise_over_surfaces": t["planarise"]["median"] / t["surfaces"]["median"]}
        print(json.dumps(case), file=sys.stderr, flush=True)
        assert equal, "the three routes differ"                    # nothing is reported of routes that disagree
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
