"""The cadence renderer on decoder surfaces (kfm_render with NV12 / P010 descriptors, csrc/render_surface_kernels.hip) measured on an
MI355X; writes profiles/surface_render.json.  Reported, not gated.

  1920x1080, 1 024 source frames resident in HBM, NV12 (8-bit) and P010 (10 bits in the high bits of 16-bit containers, RANDOM low bits).
  Plans as in tools/kfm_render_bench.py: all-24p, all-30p, all-60i, each with thresh -1 and with thresh 4.  Times are the context's HIP
  events around the kernel launches of a call (Context.profile), median [min - max] of 7 after 2 warm-up calls; bytes are algorithmic, as
  there.  Three routes to the same pictures, timed alternating in the same run:

    (a) surfaces   the in-kind render: surfaces in, surfaces out (kfm_render_surfaces_kernel);
    (b) planar     the planar kernel (kfm_render_kernel) on a planar LSB copy of the same pictures -- the path before: the same bytes
                   moved, the yardstick for whether interleaved rows or packed shifts cost anything;
    (c) planarise  the only route from surfaces before: weave_fields(nv12=True[, msb=True]) of ALL source frames into planar LSB frames
                   (weave_fields_kernel), then (b).  Its time is the sum of the two kernels; it ENDS IN PLANAR FRAMES, which an encoder
                   that takes surfaces cannot use, and there was no way back.

  Before any timing the three outputs are compared at the timed size: (a) >> s de-interleaved equals (b) equals (c) in every container
  (s = 6 for P010, 0 for NV12), and for P010 every interpolated row of (a) has zero low bits and every copied row is its source row.

    python tools/surface_render_bench.py [--out profiles/surface_render.json] [--frames 1024]
There is no CPU path: without a GPU this fails."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kfm_render_bench import H, REPS, THRESH, W, WARMUP, algorithmic_bytes, kernel_ms, rates, spread  # noqa: E402


def surfaces(A, torch, n, bits, msb, seed=None):
    """NV12-layout surfaces: Y (n, H, W) and UV (n, H / 2, W) of one container type; seed: random containers (MSB: random low bits too)"""
    dt = torch.uint8 if bits <= 8 else torch.int16
    if seed is None:
        mk = lambda h: torch.empty((n, h, W), dtype=dt, device="cuda")
    else:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed)
        lo, hi = (0, 256) if bits <= 8 else (-32768, 32768) if msb else (0, 1 << bits)
        mk = lambda h: torch.randint(lo, hi, (n, h, W), dtype=dt, device="cuda", generator=gen)
    return A.DeviceSurfaces(mk(H), mk(H // 2), None, W, H, bits, True, msb)


def planar(A, torch, n, bits):
    dt = torch.uint8 if bits <= 8 else torch.int16
    mk = lambda h, w: torch.empty((n, h, w), dtype=dt, device="cuda")
    return A.DeviceClip(mk(H, W), mk(H // 2, W // 2), mk(H // 2, W // 2), W, H, bits)


def samples(torch, t, s):
    """containers >> s of an int16 / uint8 tensor, as int32"""
    return t.to(torch.int32) if t.dtype == torch.uint8 else (t.to(torch.int32) & 0xFFFF) >> s


def routes_equal(torch, plan, s, src, out_a, out_b, out_c):
    """the identity of DESIGN.md section 6d at the timed size, frame by frame (no whole-clip temporaries)"""
    low = (1 << s) - 1
    for k in range(len(plan)):
        kind, top, bottom = (int(v) for v in tuple(plan[k])[:3])
        a = (samples(torch, out_a.Y[k], s), samples(torch, out_a.U[k, :, 0::2], s), samples(torch, out_a.U[k, :, 1::2], s))
        for x, pb, pc in zip(a, (out_b.Y[k], out_b.U[k], out_b.V[k]), (out_c.Y[k], out_c.U[k], out_c.V[k])):
            if not (torch.equal(x, samples(torch, pb, 0)) and torch.equal(pb, pc)):
                return False
        for P, Q in ((out_a.Y, src.Y), (out_a.U, src.U)):
            for parity, frame in ((0, top), (1, bottom)):
                copied = kind == 0 or parity == (kind == 2)
                rows = P[k, parity::2]
                if copied and not torch.equal(rows, Q[frame, parity::2]):
                    return False
                if not copied and low and bool(((rows.to(torch.int32) & low) != 0).any()):
                    return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_render.json"))
    ap.add_argument("--frames", type=int, default=1024)
    args = ap.parse_args()
    import torch
    import amatsukaze_amd as A
    N = args.frames
    ctx = A.Context(0)
    ctx.profile(True)
    res = {"what": "kfm_render on decoder surfaces, %dx%d, %d source frames in HBM; HIP events around the launches, median [min - max] of %d after %d "
                   "warm-up calls; bytes are algorithmic (tools/surface_render_bench.py); routes: surfaces = in kind, planar = the planar kernel on a "
                   "planar LSB copy, planarise = weave_fields of every source frame + the planar kernel (ends in planar frames)" % (W, H, N, REPS, WARMUP),
           "device": torch.cuda.get_device_name(0), "peak_TB_per_s": 8.0, "guide_copy_TB_per_s": 6.29, "cases": []}
    plans = {
        "all-24p": A.kfm_render_plan([1] * N, [n % 5 for n in range(N)]),
        "all-30p": A.kfm_render_plan([2] * N, [0] * N),
        "all-60i": A.kfm_render_plan([0] * N, [0] * N),
    }
    for layout, bits, msb in (("NV12", 8, False), ("P010", 10, True)):
        es = 1 if bits <= 8 else 2
        s = 16 - bits if msb else 0
        frame_bytes = (W * H + 2 * (W // 2) * (H // 2)) * es
        src = surfaces(A, torch, N, bits, msb, seed=91 + bits)
        src_planar = planar(A, torch, N, bits)                    # (b) reads it; (c) rewrites it with the same samples on every call

        def planarise():
            A.weave_fields(ctx, src.Y, src.U, None, src_planar, nv12=True, msb=msb)
            ctx.synchronize()

        planarise()
        for name in ("all-24p", "all-30p", "all-60i"):
            plan = plans[name]
            nout = len(plan)
            out_a, out_b, out_c = surfaces(A, torch, nout, bits, msb), planar(A, torch, nout, bits), planar(A, torch, nout, bits)
            for thresh in (-1, THRESH):
                render_a = lambda: A.kfm_render(ctx, src, plan, out_a, thresh=thresh)
                render_b = lambda: A.kfm_render(ctx, src_planar, plan, out_b, thresh=thresh)
                render_c = lambda: A.kfm_render(ctx, src_planar, plan, out_c, thresh=thresh)
                render_a(); render_b(); planarise(); render_c()
                equal = routes_equal(torch, plan, s, src, out_a, out_b, out_c)
                ms = {"surfaces": [], "planar": [], "planarise": []}
                for i in range(WARMUP + REPS):
                    ta = kernel_ms(ctx, "kfm_render_surfaces_kernel", render_a)
                    tb = kernel_ms(ctx, "kfm_render_kernel", render_b)
                    tc = kernel_ms(ctx, "weave_fields_kernel", planarise) + kernel_ms(ctx, "kfm_render_kernel", render_c)
                    if i >= WARMUP:
                        ms["surfaces"].append(ta); ms["planar"].append(tb); ms["planarise"].append(tc)
                nbytes = algorithmic_bytes([tuple(int(v) for v in e) for e in plan], frame_bytes, thresh, N)
                t = {k: spread(v) for k, v in ms.items()}
                d = t["surfaces"]["median"] - t["planar"]["median"]
                case = {"layout": layout, "bits": bits, "plan": name, "thresh": thresh, "source_frames": N, "output_frames": nout,
                        "algorithmic_bytes": nbytes, "outputs_of_the_three_routes_equal": bool(equal),
                        "surfaces": {"ms": t["surfaces"], **rates(nbytes, t["surfaces"])},
                        "planar": {"ms": t["planar"], **rates(nbytes, t["planar"])},
                        "planarise_then_planar": {"ms": t["planarise"], "ends_in": "planar frames"},
                        "surfaces_minus_planar_ms": d, "surfaces_minus_planar_share": d / t["planar"]["median"],
                        "surfaces_outside_planar_spread": bool(not t["planar"]["min"] <= t["surfaces"]["median"] <= t["planar"]["max"]),
                        "planarise_over_surfaces": t["planarise"]["median"] / t["surfaces"]["median"]}
                res["cases"].append(case)
                print(json.dumps(case), file=sys.stderr, flush=True)
                assert equal, "the three routes differ"
            del out_a, out_b, out_c
            torch.cuda.empty_cache()
        del src, src_planar
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
