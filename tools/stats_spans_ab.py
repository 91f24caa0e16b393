"""frame_stats_kernel, one library against another (profiles/stats_spans_notes.md): per shape the mean time of eight launches from the
context's kernel timers, and a hash of every record.  One run of `--child` is one repetition of one library (AMTGPU_LIB picks it, as in
tools/tile_bench.py); a job alternates the libraries, every run under a time limit of its own, and appends the lines to one file:
    for rep in 1 2 3 4 5; do for lib in parent change; do
      AMTGPU_LIB=amatsukaze_amd/libamt_gpu_stats_$lib.so AMT_AB_TAG=$lib timeout -k 10 300 python tools/stats_spans_ab.py --child >> ab.jsonl || exit 1
    done; done
    python tools/stats_spans_ab.py --summary ab.jsonl
Counter passes (rocprofv3 --pmc, nothing else in the run) take fewer frames and launches: AMT_STATS_FRAMES=2048 AMT_STATS_LAUNCHES=2, then
    python tools/stats_spans_ab.py --counters <directory with one rocprofv3 output directory per library> <frames>
The libraries are copies built by amatsukaze_amd/build.py build_variant (the parent's from a checkout of the parent commit)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
# (tag: width, height, bits, pitch in samples, frames)
SHAPES = {"1440x1080_8bit_p1472": (1440, 1080, 8, 1472, 10000), "1920x1080_8bit": (1920, 1080, 8, 1920, 4096),
          "1920x1080_10bit": (1920, 1080, 10, 1920, 4096)}


def shapes():
    cap = int(os.environ.get("AMT_STATS_FRAMES", "0"))
    return {k: v[:4] + (min(v[4], cap) if cap else v[4],) for k, v in SHAPES.items()}


def child():
    import hashlib
    import torch
    import amt_synth as S
    from amatsukaze_amd import Context, FrameStats
    ctx = Context(0)
    dev = torch.device("cuda:0")
    launches = int(os.environ.get("AMT_STATS_LAUNCHES", "8"))
    out = {"lib": os.environ.get("AMT_AB_TAG", "default")}
    for tag, (W, H, bits, pitch, N) in shapes().items():
        Y = S.make_clip_torch(N, W, H, 0x5EED0002, None, None, 0, 0, dev, bits=bits, pitchY=pitch, chroma=False)["Y"]
        fs = FrameStats(ctx, W, H, bits)
        o = torch.zeros((N, 8), dtype=torch.int64, device=dev)
        fs.run_device(Y, o)
        torch.cuda.synchronize()
        ctx.profile(True)
        for _ in range(launches):
            fs.run_device(Y, o)
        torch.cuda.synchronize()
        c, ms = ctx.profile_report()["frame_stats_kernel"]
        ctx.profile(False)
        out[tag] = {"ms": ms / c, "frames": N, "sha": hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest()[:16]}
        del Y, o
    print(json.dumps(out), flush=True)


def summary(path):
    import statistics
    runs = [json.loads(l) for l in open(path) if l.startswith("{")]
    libs = sorted({r["lib"] for r in runs})
    res = {}
    for tag in SHAPES:
        shas = {r[tag]["sha"] for r in runs}
        res[tag] = {"records_identical": len(shas) == 1}
        for lib in libs:
            ms = [r[tag]["ms"] for r in runs if r["lib"] == lib]
            res[tag][lib] = {"ms": ms, "median": statistics.median(ms), "min": min(ms), "max": max(ms)}
    print(json.dumps(res, indent=1))


def counters(root, frames):
    """per library directory under root: every counter of the frame_stats dispatches, per 128-byte line of the launch's frames and per frame
    (the child's launches in order: 1 + AMT_STATS_LAUNCHES per shape)"""
    import collections, csv, glob
    res = {}
    for lib in sorted(os.listdir(root)):
        agg = collections.defaultdict(list)
        for f in glob.glob(os.path.join(root, lib, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                if "frame_stats" in r.get("Kernel_Name", ""):
                    agg[r["Counter_Name"]].append((int(r["Dispatch_Id"]), float(r["Counter_Value"])))
        res[lib] = {}
        for c, rows in sorted(agg.items()):
            rows.sort()
            per = len(rows) // len(SHAPES)
            for i, (tag, (W, H, bits, pitch, N)) in enumerate(SHAPES.items()):
                v = [x for _, x in rows[per * i:per * i + per]]
                n = min(N, frames)
                lines = n * W * H * (1 if bits <= 8 else 2) / 128
                res[lib].setdefault(tag, {})[c] = {"mean": sum(v) / len(v), "per_line": sum(v) / len(v) / lines, "per_frame": sum(v) / len(v) / n}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    elif "--summary" in sys.argv:
        summary(sys.argv[sys.argv.index("--summary") + 1])
    elif "--counters" in sys.argv:
        i = sys.argv.index("--counters")
        counters(sys.argv[i + 1], int(sys.argv[i + 2]))
