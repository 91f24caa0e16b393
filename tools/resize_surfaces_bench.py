"""The resize on decoder surfaces (Resizer.run with NV12 / P010 descriptors, csrc/resize_surface_kernels.hip) measured on an MI355X;
writes profiles/resize_surfaces.json.  Reported, not gated.

  1920x1080 -> 1280x720, 1 024 frames resident in HBM, Blackman taps 4 (the server's BlackmanResize(1280, 720)), the default scratch;
  NV12 (8-bit) and P010 (10 bits in the high bits of 16-bit containers, RANDOM low bits), random samples.  Times are the context's HIP
  events around the kernel launches of a call (Context.profile; a stage's launches of all rounds summed), median [min - max] of 7 after
  2 warm-up calls.  Three routes to the same pictures, timed alternating in the same run:

    (a) surfaces   the in-kind resize: surfaces in, surfaces out (resize_surface_h_kernel, resize_surface_v_kernel);
    (b) planar     the planar kernels (resize_h_kernel, resize_v_kernel) on a planar LSB copy of the same pictures -- the same rule on the
                   same samples, the yardstick for what the pair staging and the shifts cost;
    (c) planarise  the only route from surfaces before: amtgpu_surfaces_extract_rect(0, 0, W, H) of ALL frames into planar LSB frames
                   (surfaces_extract_kernel), then (b).  Its time is the sum; it ENDS IN PLANAR FRAMES and holds a second copy of the clip.

  Before any figure is reported the three outputs are compared at the timed size: (a) >> s de-interleaved equals (b) equals (c) in every
  container (s = 6 for P010, 0 for NV12), every container of (a) has zero low bits, and frames 0, the middle one and the last of (a)
  equal the numpy restatement (tests/resize_surfaces_ref.py).  Beside the times, from hipcc's assembly: each timed form's registers and
  the vector instructions per output sample of each stage, counted as tools/resize_bench.py counts the planar forms' (horizontal: the
  tap section of the row loop plus one pass of the 16-byte staging loop per wave and row -- the luma path for luma runs, the pair path
  for UV runs; vertical: the walk body per tap times K plus the store section).

    python tools/resize_surfaces_bench.py [--out profiles/resize_surfaces.json] [--frames 1024] [--isa-only]
There is no CPU path: without a GPU this fails (but for --isa-only)."""
import argparse
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kfm_render_bench import H, REPS, W, WARMUP, spread  # noqa: E402
from resize_bench import DH, DW, blocks_of, valu  # noqa: E402
from surface_render_bench import planar, samples, surfaces  # noqa: E402

K = 12                                           # of every axis of 1920x1080 -> 1280x720 (checked in main)


def tap_paths(body, es):
    """(vector instructions of the tap section along the luma path, along the pair path) of a horizontal form: the section runs from
    the first LDS read to the store; where the form has two tap paths (interleaved) they are the two blocks with four or more 24-bit
    multiplies -- the pair path's LDS reads are all single containers at multiples of 2 * es -- and the rest is common to both"""
    first = next(i for i, l in enumerate(body) if l.startswith("ds_read"))
    last = max(i for i, l in enumerate(body) if re.match(r"global_store_(byte|short)", l))
    bl = blocks_of(body[first:last + 1])
    reads = lambda b: [l for l in b if l.startswith("ds_read")]
    muls = lambda b: sum(bool(re.match(r"v_(mul|mad)_i32_i24", l)) for l in b)
    taps = [b for b in bl if muls(b) >= 4]
    common = sum(valu(b) for b in bl if muls(b) < 4)
    if len(taps) == 1:
        return common + valu(taps[0]), None
    assert len(taps) == 2, len(taps)

    def is_pair(b):
        offs = [int(m.group(1)) if (m := re.search(r"offset:(\d+)", l)) else 0 for l in reads(b)]
        return all(re.match(r"ds_read_u(8|16) ", l) for l in reads(b)) and all(o % (2 * es) == 0 for o in offs)

    (pair,), (luma,) = [b for b in taps if is_pair(b)], [b for b in taps if not is_pair(b)]
    return common + valu(luma), common + valu(pair)


def kernel_isa():
    """{form: registers and the vector instructions of its hot sections} for the forms the timed cases run, planar ones beside them"""
    from test_isa_guards import kernels_of
    from test_isa_surfaces import compile_file
    res = {}
    forms = (("resize_kernels.hip", "resize_h_kernelIhLi12E", "resize_v_kernelIhLb1E", "planar, 8-bit", 1),
             ("resize_kernels.hip", "resize_h_kernelItLi12E", "resize_v_kernelItLb1E", "planar, 16-bit", 2),
             ("resize_surface_kernels.hip", "resize_surface_h_kernelIhLi12ELb0ELb1E", "resize_surface_v_kernelIhLb1ELb0E", "NV12", 1),
             ("resize_surface_kernels.hip", "resize_surface_h_kernelItLi12ELb1ELb1E", "resize_surface_v_kernelItLb1ELb1E", "P010", 2))
    asms = {}
    for name, htag, vtag, form, es in forms:
        ks = asms.setdefault(name, kernels_of(compile_file(name)))
        (hk,) = [k for n, k in ks.items() if htag in n]
        (vk,) = [k for n, k in ks.items() if vtag in n]
        hb, vb = [l.strip() for l in hk["body"]], [l.strip() for l in vk["body"]]
        luma, pair = tap_paths(hb, es)
        stage = next(b for b in blocks_of(hb) if any(l.startswith("ds_write_b128") for l in b))
        bl = blocks_of(vb)
        walk = max(bl, key=lambda b: sum(l.startswith("global_load_dwordx4") for l in b))
        taps = sum(l.startswith("global_load_dwordx4") for l in walk)
        store = next(b for b in bl if any(l.startswith("global_store_dwordx4") for l in b))
        px = 16 // es
        # wave-instructions per frame over output samples per frame, idle lanes of partly filled waves counted as issued
        luma_waves, chroma_waves = -(-DW // 64) * H, 2 * -(-(DW // 2) // 64) * (H // 2)
        if pair is not None:
            chroma_waves = -(-(DW // 2) // 32) * (H // 2)                  # one UV plane, 32 pairs to a wave
        h_per_sample = (luma_waves * (luma + valu(stage)) + chroma_waves * ((luma if pair is None else pair) + valu(stage))) * 64 / (DW * H * 3 // 2)
        v_waves = sum(-(-(-(-dw // px)) // 64) * dh for dw, dh in ((DW, DH), (DW // 2, DH // 2), (DW // 2, DH // 2)))
        if pair is not None:
            v_waves = sum(-(-(-(-dw // px)) // 64) * dh for dw, dh in ((DW, DH), (DW, DH // 2)))
        v_per_wave = valu(walk) / taps * K + valu(store)
        res[form] = {"horizontal": {"vgprs": hk["meta"]["vgpr_count"], "tap_section_vector_instructions_luma_path": luma,
                                    "tap_section_vector_instructions_pair_path": pair, "staging_pass_vector_instructions": valu(stage),
                                    "vector_instructions_per_output_sample": h_per_sample},
                     "vertical": {"vgprs": vk["meta"]["vgpr_count"], "walk_body_taps": taps, "walk_body_vector_instructions": valu(walk),
                                  "store_section_vector_instructions": valu(store),
                                  "vector_instructions_per_output_sample": v_per_wave * v_waves * 64 / (DW * DH * 3 // 2)}}
    return res


def sized(A, torch, n, w, h, bits, msb, kind):
    """an uninitialised clip of w x h: kind "surfaces" (NV12 layout) or "planar\""""
    dt = torch.uint8 if bits <= 8 else torch.int16
    mk = lambda hh, ww: torch.empty((n, hh, ww), dtype=dt, device="cuda")
    if kind == "surfaces":
        return A.DeviceSurfaces(mk(h, w), mk(h // 2, w), None, w, h, bits, True, msb)
    return A.DeviceClip(mk(h, w), mk(h // 2, w // 2), mk(h // 2, w // 2), w, h, bits)


def stages_ms(ctx, names, call):
    """{kernel: ms} of the launches of the named kernels inside call() (HIP events, all launches of a name summed)"""
    before = {k: ctx.profile_report().get(k, (0, 0.0)) for k in names}
    call()
    after = {k: ctx.profile_report()[k] for k in names}
    assert all(after[k][0] > before[k][0] for k in names), (names, before, after)
    return {k: after[k][1] - before[k][1] for k in names}


def routes_equal(torch, s, out_a, out_b, out_c):
    low = (1 << s) - 1
    for k in range(out_a.num_frames):
        a = (samples(torch, out_a.Y[k], s), samples(torch, out_a.U[k, :, 0::2], s), samples(torch, out_a.U[k, :, 1::2], s))
        for x, pb, pc in zip(a, (out_b.Y[k], out_b.U[k], out_b.V[k]), (out_c.Y[k], out_c.U[k], out_c.V[k])):
            if not (torch.equal(x, samples(torch, pb, 0)) and torch.equal(pb, pc)):
                return False
        if low and any(bool(((P[k].to(torch.int32) & low) != 0).any()) for P in (out_a.Y, out_a.U)):
            return False
    return True


def check_frames(np, RS, src, out_a, bits, msb):
    dt = np.uint8 if bits <= 8 else np.uint16
    host = lambda t: t.cpu().numpy().view(dt)
    n = src.num_frames
    frames = sorted({0, n // 2, n - 1})
    for f in frames:
        want = RS.resize_surfaces((host(src.Y[f:f + 1]), host(src.U[f:f + 1])), DW, DH, bits, True, msb)
        for g, w_ in zip((out_a.Y, out_a.U), want):
            assert np.array_equal(host(g[f:f + 1]), w_), ("output frame", f)
    return len(frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_surfaces.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--isa-only", action="store_true", help="print the registers and instruction counts and stop (needs no GPU)")
    args = ap.parse_args()
    import resize_ref as R
    assert K == R.program(W, DW)[0] == R.program(H, DH)[0] == R.program(W // 2, DW // 2)[0] == R.program(H // 2, DH // 2)[0]
    isa = kernel_isa()
    if args.isa_only:
        print(json.dumps(isa, indent=1))
        return
    import numpy as np
    import torch
    import amatsukaze_amd as A
    import resize_surfaces_ref as RS
    from amatsukaze_amd.api import _p
    N = args.frames
    ctx = A.Context(0)
    ctx.profile(True)
    res = {"what": "Resizer on decoder surfaces, %dx%d -> %dx%d (Blackman, taps 4, K %d), %d frames in HBM, default scratch; HIP events around the "
                   "launches, median [min - max] of %d after %d warm-up calls (tools/resize_surfaces_bench.py); routes: surfaces = in kind, planar = "
                   "the planar kernels on a planar LSB copy, planarise = amtgpu_surfaces_extract_rect of every frame + the planar kernels (ends in "
                   "planar frames, holds a second copy of the clip)" % (W, H, DW, DH, K, N, REPS, WARMUP),
           "device": torch.cuda.get_device_name(0), "isa": isa, "cases": []}
    HS, VS, HP, VP, EX = "resize_surface_h_kernel", "resize_surface_v_kernel", "resize_h_kernel", "resize_v_kernel", "surfaces_extract_kernel"
    for layout, bits, msb in (("NV12", 8, False), ("P010", 10, True)):
        s = 16 - bits if msb else 0
        es = 1 if bits <= 8 else 2
        src = surfaces(A, torch, N, bits, msb, seed=61 + bits)
        src_planar = planar(A, torch, N, bits)                        # (b) reads it; (c) rewrites it with the same samples on every call
        d = src.ref()

        def planarise():
            P = src_planar
            ctx.check(ctx.lib.amtgpu_surfaces_extract_rect(ctx.h, C.byref(d), 0, 0, W, H, N, _p(P.Y), _p(P.U), _p(P.V), int(P.Y.stride(0)) * es,
                                                           int(P.U.stride(0)) * es, int(P.Y.stride(1)), int(P.U.stride(1))), "extract_rect")
            ctx.synchronize()

        planarise()
        out_a = sized(A, torch, N, DW, DH, bits, msb, "surfaces")
        out_b, out_c = sized(A, torch, N, DW, DH, bits, msb, "planar"), sized(A, torch, N, DW, DH, bits, msb, "planar")
        rz = A.Resizer(ctx, (W, H), (DW, DH), bits)
        run_a, run_b, run_c = (lambda: rz.run(src, out_a)), (lambda: rz.run(src_planar, out_b)), (lambda: rz.run(src_planar, out_c))
        run_a(); run_b(); planarise(); run_c()
        equal = routes_equal(torch, s, out_a, out_b, out_c)
        checked = check_frames(np, RS, src, out_a, bits, msb)
        ms = {r: {"horizontal": [], "vertical": [], "total": []} for r in ("surfaces", "planar", "planarise")}
        for i in range(WARMUP + REPS):
            ta = stages_ms(ctx, (HS, VS), run_a)
            tb = stages_ms(ctx, (HP, VP), run_b)
            te = stages_ms(ctx, (EX,), planarise)[EX]
            tc = stages_ms(ctx, (HP, VP), run_c)
            if i >= WARMUP:
                for route, h, v, extra in (("surfaces", ta[HS], ta[VS], 0.0), ("planar", tb[HP], tb[VP], 0.0), ("planarise", tc[HP], tc[VP], te)):
                    ms[route]["horizontal"].append(h); ms[route]["vertical"].append(v); ms[route]["total"].append(h + v + extra)
        t = {r: {k: spread(v) for k, v in st.items()} for r, st in ms.items()}
        apart = lambda x, y: bool(x["max"] < y["min"] or y["max"] < x["min"])
        case = {"layout": layout, "bits": bits, "frames": N, "outputs_of_the_three_routes_equal": bool(equal), "frames_checked_against_numpy": checked,
                "surfaces": {"ms": t["surfaces"]}, "planar": {"ms": t["planar"]},
                "planarise_then_planar": {"ms": t["planarise"], "ends_in": "planar frames"}}
        for stage in ("horizontal", "vertical", "total"):
            a, b, c = t["surfaces"][stage], t["planar"][stage], t["planarise"][stage]
            case["surfaces_vs_planar_" + stage] = {"difference_ms": a["median"] - b["median"], "share": (a["median"] - b["median"]) / b["median"],
                                                   "ranges_apart": apart(a, b)}
        case["planarise_over_surfaces_total"] = t["planarise"]["total"]["median"] / t["surfaces"]["total"]["median"]
        case["planarise_vs_surfaces_ranges_apart"] = apart(t["planarise"]["total"], t["surfaces"]["total"])
        print(json.dumps(case), file=sys.stderr, flush=True)
        assert equal, "the three routes differ"                       # nothing is reported of such a run
        res["cases"].append(case)
        rz.close()
        del src, src_planar, out_a, out_b, out_c
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
