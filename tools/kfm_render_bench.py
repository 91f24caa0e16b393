"""The cadence renderer (kfm_render, csrc/render_kernels.hip) measured on an MI355X; writes profiles/kfm_render.json.

  1920x1080 at 8 and at 10 bits, 1 024 source frames resident in HBM (3.2 / 6.4 GB; with the destination far above the 256 MiB Infinity
  Cache, so nothing a launch reads or writes is left there by the launch before).  Plans: all-24p (820 woven frames, a fifth of them from
  two source frames), all-30p (1 024 frames copied), all-60i (2 048 bobbed fields) with thresh -1 and with thresh 4.  Times are the
  context's HIP events around the one kernel launch of a call (Context.profile), median [min - max] of 7 after 2 warm-up calls.

  Algorithmic bytes of an output frame of F bytes: every source row the rule reads, counted once, plus the rows written.
      WEAVE                          F read (each row from one of the two frames)                       + F written = 2 F
      BOB, thresh < 0                F / 2 read (the kept rows; every up / dn row is one of them)        + F written = 1.5 F
      BOB, thresh >= 0               F / 2 kept + F / 2 of frame n's other field + F / 2 of the neighbour frame's (none at a clip end)
                                                                                                        + F written = 2.5 F (2 F at the ends)
  The kernel ISSUES more loads than that for a bob (each up / dn row is loaded by the two missing rows next to it and by its own copy); what
  of that reaches HBM is not measured here.  Rates are algorithmic bytes / time, as TB/s and as a share of the 8 TB/s peak; the float4 copy
  the kernel guide measured reaches 6.29 TB/s (79 %).

  For the two weave-only plans amtgpu_weave_fields_batch -- the only other route to those frames -- is timed with the plan's top / bottom
  arrays over the same source into a second destination, alternating with the new call in the same run; the two destinations must be equal.
  Two bobbed fields per case are checked against the numpy restatement (tests/kfm_render_ref.py) before any timing.

    python tools/kfm_render_bench.py [--out profiles/kfm_render.json] [--frames 1024]
There is no CPU path: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1920, 1080
HBM_PEAK, COPY_MEASURED = 8e12, 6.29e12
REPS, WARMUP = 7, 2
THRESH = 4


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def kernel_ms(ctx, name, call):
    """HIP-event time of the launch(es) of kernel `name` inside call()"""
    before = ctx.profile_report().get(name, (0, 0.0))
    call()
    after = ctx.profile_report()[name]
    assert after[0] == before[0] + 1, (name, before, after)
    return after[1] - before[1]


def algorithmic_bytes(plan, frame_bytes, thresh, clip_frames):
    total = 0.0
    for kind, top, _, _ in plan:
        if kind == 0:
            total += 2.0 * frame_bytes
        elif thresh < 0:
            total += 1.5 * frame_bytes
        else:
            at_end = (kind == 1 and top == 0) or (kind == 2 and top == clip_frames - 1)
            total += (2.0 if at_end else 2.5) * frame_bytes
    return total


def rates(nbytes, t):
    r = nbytes / (t["median"] * 1e-3)
    return {"TB_per_s": r / 1e12, "share_of_8TBps_peak": r / HBM_PEAK, "share_of_measured_copy_6.29TBps": r / COPY_MEASURED}


def clip(A, torch, n, bits, seed=None):
    dt = torch.uint8 if bits <= 8 else torch.int16
    if seed is None:
        mk = lambda h, w: torch.empty((n, h, w), dtype=dt, device="cuda")
    else:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed)
        mk = lambda h, w: torch.randint(0, 1 << bits, (n, h, w), dtype=dt, device="cuda", generator=gen)
    return A.DeviceClip(mk(H, W), mk(H // 2, W // 2), mk(H // 2, W // 2), W, H, bits)


def check_bobs(np, R, src, dst, plan, thresh, bits):
    """output frames 0, 1 and the middle pair against the numpy restatement"""
    dt = np.uint8 if bits <= 8 else np.uint16
    host = lambda t: t.cpu().numpy().view(dt)
    n = src.num_frames
    for k in (0, 1, len(plan) // 2, len(plan) // 2 + 1):
        e = tuple(int(v) for v in plan[k])
        lo, hi = max(0, e[1] - 1), min(n, e[1] + 2)
        planes = tuple(host(p[lo:hi]) for p in (src.Y, src.U, src.V))
        want = R.render_frame_ref(planes, e, lo, n, thresh)
        for g, w_ in zip((dst.Y, dst.U, dst.V), want):
            assert np.array_equal(host(g[k]), w_), ("output frame", k, e)
    return 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfm_render.json"))
    ap.add_argument("--frames", type=int, default=1024)
    args = ap.parse_args()
    import numpy as np
    import torch
    import amatsukaze_amd as A
    import kfm_render_ref as R
    N = args.frames
    ctx = A.Context(0)
    ctx.profile(True)
    res = {"what": "kfm_render_kernel, %dx%d, %d source frames in HBM; HIP events around the launch, median [min - max] of %d after %d warm-up calls; "
                   "bytes are algorithmic (tools/kfm_render_bench.py)" % (W, H, N, REPS, WARMUP),
           "device": torch.cuda.get_device_name(0), "peak_TB_per_s": 8.0, "guide_copy_TB_per_s": 6.29, "cases": []}
    plans = {
        "all-24p": A.kfm_render_plan([1] * N, [n % 5 for n in range(N)]),
        "all-30p": A.kfm_render_plan([2] * N, [0] * N),
        "all-60i": A.kfm_render_plan([0] * N, [0] * N),
    }
    for bits in (8, 10):
        es = 1 if bits <= 8 else 2
        frame_bytes = (W * H + 2 * (W // 2) * (H // 2)) * es
        src = clip(A, torch, N, bits, seed=77 + bits)
        for name, thresh in (("all-24p", -1), ("all-30p", -1), ("all-60i", -1), ("all-60i", THRESH)):
            plan = plans[name]
            nout = len(plan)
            dst = clip(A, torch, nout, bits)
            weave_only = name != "all-60i"
            dst2 = clip(A, torch, nout, bits) if weave_only else None
            top, bottom = [int(v) for v in plan["top"]], [int(v) for v in plan["bottom"]]
            render = lambda: A.kfm_render(ctx, src, plan, dst, thresh=thresh)

            def weave():
                A.weave_fields(ctx, src.Y, src.U, src.V, dst2, top, bottom)
                ctx.synchronize()

            render()
            checked = 0
            if weave_only:
                weave()
                assert all(torch.equal(a, b) for a, b in ((dst.Y, dst2.Y), (dst.U, dst2.U), (dst.V, dst2.V))), "kfm_render and weave_fields differ"
            else:
                checked = check_bobs(np, R, src, dst, plan, thresh, bits)
            ms, ms_weave = [], []
            for i in range(WARMUP + REPS):
                t = kernel_ms(ctx, "kfm_render_kernel", render)
                tw = kernel_ms(ctx, "weave_fields_kernel", weave) if weave_only else None
                if i >= WARMUP:
                    ms.append(t)
                    if weave_only:
                        ms_weave.append(tw)
            nbytes = algorithmic_bytes([tuple(int(v) for v in e) for e in plan], frame_bytes, thresh, N)
            t = spread(ms)
            case = {"plan": name, "bits": bits, "thresh": thresh, "source_frames": N, "output_frames": nout, "source_bytes": N * frame_bytes,
                    "destination_bytes": nout * frame_bytes, "algorithmic_bytes": nbytes, "ms": t, **rates(nbytes, t),
                    "bobbed_fields_checked_against_numpy": checked}
            if weave_only:
                tw = spread(ms_weave)
                case["weave_fields_batch"] = {"ms": tw, **rates(nbytes, tw), "outputs_equal": True}
                case["render_minus_weave_ms"] = t["median"] - tw["median"]
                case["render_slower_than_weave_by_more_than_weave_spread"] = bool(t["median"] - tw["median"] > tw["max"] - tw["min"])
            res["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
            del dst, dst2
            torch.cuda.empty_cache()
        del src
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
