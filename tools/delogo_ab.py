#!/usr/bin/env python3
"""A/B of Delogo between two builds of the library (profiles/delogo_unify.json): by default the parent commit's against this tree's.

Each library is loaded by child processes of this script through AMTGPU_LIB, parent and branch alternating, --children (5) per library, one
process each under a time limit of its own; the first child that fails ends the run.  A child times every shape: the `delogo_kernel`
profile span of 10 in-place launches after a warm-up launch, the rectangles restored in between, and the SHA-256 of the rectangles after
one erase.

Shapes, all with a 256x128 logo and the fades CalcFade gives the bench's 8-bit clip (54 % of the frames have a non-zero fade):
  bench_8bit          10 000 frames of 1440x1080 8-bit, logo at (1120, 64): bench.py's clip and call
  bench_8bit_x1122    the same frames, logo at (1122, 64): luma rows start 2 (mod 4) samples in, odd chroma origin
  hd_10bit            4 000 frames of 1920x1080 10-bit noise, logo at (1600, 64), resident next to the 8-bit clip

Per shape and library: median, min and max over the children of the time per launch, and the SHA.  Criteria per shape: the SHAs are
equal, and branch median <= parent median + (parent max - parent min).

The parent's library is built from a checkout of the parent commit and placed next to this tree's:
    git worktree add --detach ../parent HEAD~1 && python ../parent/amatsukaze_amd/build.py
    cp ../parent/amatsukaze_amd/libamt_gpu.so amatsukaze_amd/libamt_gpu_parent.so
    python tools/delogo_ab.py --out profiles/delogo_unify.json [--parent LIB] [--branch LIB]          (on the GPU box)"""
import argparse, hashlib, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
LIBS = {"parent": os.path.join(ROOT, "amatsukaze_amd", "libamt_gpu_parent.so"), "branch": os.path.join(ROOT, "amatsukaze_amd", "libamt_gpu.so")}
N8, N10, LAUNCHES = 10000, 4000, 10


def child():
    import torch
    import amt_synth as S
    import bench
    from amatsukaze_amd import AMTAnalyzeLogo, AMTEraseLogo, Context, DeviceClip, Logo
    dev = torch.device("cuda:0")
    ctx = Context(0)
    logos_np, alpha, alphaUV = bench.make_logos()
    LW, LH = bench.LW, bench.LH

    def run(clip, W, H, X, Y0, d_f):
        er = AMTEraseLogo(ctx, Logo.from_planes(ctx, logos_np[0], LW, LH, W, H, X, Y0), "", 0, 16)
        rects = [clip.Y[:, Y0:Y0 + LH, X:X + LW], clip.U[:, Y0 // 2:(Y0 + LH) // 2, X // 2:(X + LW) // 2], clip.V[:, Y0 // 2:(Y0 + LH) // 2, X // 2:(X + LW) // 2]]
        keep = [t.clone() for t in rects]

        def restore():
            for t, k in zip(rects, keep):
                t.copy_(k)
        er.erase_device_fades(clip, d_f); restore(); torch.cuda.synchronize()
        ctx.profile(True)
        for _ in range(LAUNCHES):
            er.erase_device_fades(clip, d_f)
            restore()
        torch.cuda.synchronize()
        c, ms = ctx.profile_report()["delogo_kernel"]
        ctx.profile(False)
        assert c == LAUNCHES
        er.erase_device_fades(clip, d_f); torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in rects:
            h.update(t.contiguous().cpu().numpy().tobytes())
        restore()
        return {"ms": ms / c, "sha": h.hexdigest()[:16]}

    W, H, X, Y0 = bench.W, bench.H, bench.IMGX, bench.IMGY
    c8 = S.make_clip_torch(N8, W, H, 0x5EED0002, alpha, alphaUV, X, Y0, dev, period=900, fade=12, pitchY=bench.PITCH_Y, pitchUV=bench.PITCH_UV)
    clip8 = DeviceClip(c8["Y"], c8["U"], c8["V"], W, H, 8)
    an = AMTAnalyzeLogo(ctx, Logo.from_planes(ctx, logos_np[0], LW, LH, W, H, X, Y0), bench.MASKRATIO, mode="linear")
    er = AMTEraseLogo(ctx, Logo.from_planes(ctx, logos_np[0], LW, LH, W, H, X, Y0), "", 0, 16)
    d_an = torch.empty((N8, 33), dtype=torch.float32, device=dev)
    d_f = torch.empty((N8, 2), dtype=torch.float32, device=dev)
    an.analyze_device(clip8.Y, 8, d_an)
    er.calc_fades_device(d_an, N8, out=d_f)
    res = {"nonzero_share": float((d_f.abs().sum(dim=1) != 0).float().mean())}
    res["bench_8bit"] = run(clip8, W, H, X, Y0, d_f)
    res["bench_8bit_x1122"] = run(clip8, W, H, 1122, Y0, d_f)
    g = torch.Generator(device=dev).manual_seed(0x5E10)
    planes = []
    for shape in ((N10, 1080, 1920), (N10, 540, 960), (N10, 540, 960)):
        t = torch.empty(shape, dtype=torch.int16, device=dev)
        for i in range(0, N10, 250):                                     # (randint makes int64: a chunk at a time)
            t[i:i + 250] = torch.randint(0, 1024, (min(250, N10 - i),) + shape[1:], generator=g, device=dev).to(torch.int16)
        planes.append(t)
    res["hd_10bit"] = run(DeviceClip(*planes, 1920, 1080, 10), 1920, 1080, 1600, 64, d_f[:N10].contiguous())
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delogo_unify.json"))
    ap.add_argument("--parent", default=LIBS["parent"])
    ap.add_argument("--branch", default=LIBS["branch"])
    ap.add_argument("--children", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    LIBS.update(parent=os.path.abspath(a.parent), branch=os.path.abspath(a.branch))
    for so in LIBS.values():
        if not os.path.exists(so):
            sys.exit(f"missing {so}")
    runs = {k: [] for k in LIBS}
    failed = None
    for i in range(a.children):
        for which, so in LIBS.items():
            cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child"]
            r = subprocess.run(cmd, env=dict(os.environ, AMTGPU_LIB=so), capture_output=True, text=True)
            if r.returncode != 0:
                failed = {"library": which, "child": i, "exit": r.returncode, "stderr": r.stderr[-600:]}
                break
            runs[which].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(which, i, json.dumps(runs[which][-1]), file=sys.stderr, flush=True)
        if failed:
            break
    res = {"frames": {"bench_8bit": N8, "bench_8bit_x1122": N8, "hd_10bit": N10}, "launches_per_child": LAUNCHES,
           "timing": "the delogo_kernel profile span (HIP events on the context's stream), ms per launch, one figure per child process; "
                     "parent and branch children alternate", "shapes": {}}
    if failed:
        res["failed"] = failed
    else:
        for shape in ("bench_8bit", "bench_8bit_x1122", "hd_10bit"):
            row = {}
            for which in LIBS:
                ms = [c[shape]["ms"] for c in runs[which]]
                shas = sorted({c[shape]["sha"] for c in runs[which]})
                row[which] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                              "ms": [round(x, 4) for x in ms], "sha": shas[0] if len(shas) == 1 else shas}
            p, b = row["parent"], row["branch"]
            margin = p["max_ms"] - p["min_ms"]
            row["sha_equal"] = p["sha"] == b["sha"] and isinstance(p["sha"], str)
            row["parent_spread_ms"] = round(margin, 4)
            row["branch_median_within_parent_median_plus_spread"] = bool(b["median_ms"] <= p["median_ms"] + margin)
            res["shapes"][shape] = row
        res["nonzero_share"] = runs["parent"][0]["nonzero_share"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
        sys.exit(0)
    sys.exit(main())
