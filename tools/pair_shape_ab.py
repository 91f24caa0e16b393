"""The scan pair kernel on logo lists that are NOT the bench's (tests/logo_sets.py, 352 x 240 frames of noise): ms per launch of
logo_eval_pair_kernel.scan and a hash of the records, this commit's library against another (--lib NAME: amatsukaze_amd/libamt_gpu_tile_NAME.so,
e.g. the parent commit's), alternated, a fresh process per repetition (AMTGPU_LIB).  tile_pair_shape (csrc/eval_tiles.hpp) takes the 7 + 1
shape for every list here on a model fitted to the bench's logos alone; this is the check of that choice on other masks
(profiles/pair_waves_notes.md).  python tools/pair_shape_ab.py --lib parent --reps 5 [--out FILE]"""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
NFRAMES = 16384
if "--child" in sys.argv:
    import hashlib
    import torch
    import logo_sets as LS
    from amatsukaze_amd import Context, LogoFrame
    ctx = Context(0); dev = torch.device("cuda:0")
    W, H = LS.SMALL_FRAME
    # three: LOGO_A, the tall LOGO_B and LOGO_E; tall: LOGO_B alone, bands of 6, 7, 7 and 2 tiles; short: LOGO_C, two bands of 7 and 5 tiles
    lists = {"three": [LS.LOGO_A, LS.LOGO_B, LS.LOGO_E], "tall": [LS.LOGO_B], "short": [LS.LOGO_C], "four": [LS.LOGO_A, LS.LOGO_B, LS.LOGO_C, LS.LOGO_E]}
    torch.manual_seed(0x5CA74000)
    Y = torch.randint(0, 256, (NFRAMES, H, W), dtype=torch.uint8, device=dev)
    out = {}
    for name, entries in lists.items():
        built = LS.build(entries, (W, H), ctx=ctx)
        lf = LogoFrame(ctx, built.logos, LS.MASKRATIO); lf.begin(W, H, 8, NFRAMES)
        lf.scan_batch(Y, 8, 0, NFRAMES); torch.cuda.synchronize()
        ctx.profile(True)
        for _ in range(8):
            lf.scan_batch(Y, 8, 0, NFRAMES)
        torch.cuda.synchronize()
        rep = ctx.profile_report(); ctx.profile(False)
        (ms,) = [ms / c for k, (c, ms) in rep.items() if c and "pair" in k]
        out[name] = {"pair_ms": ms, "scan_sha": hashlib.sha256(lf.evalResults.tobytes()).hexdigest()[:16]}
    print(json.dumps(out)); sys.exit(0)
names = ["default"] + [sys.argv[i + 1] for i, a in enumerate(sys.argv[:-1]) if a == "--lib"]
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
res = {n: [] for n in names}
for rep in range(REPS):
    for name in names:
        env = dict(os.environ)
        if name != "default":
            env["AMTGPU_LIB"] = os.path.join(ROOT, "amatsukaze_amd", f"libamt_gpu_tile_{name}.so")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=200)
        if r.returncode != 0:
            print(name, (r.stderr or r.stdout)[-600:], flush=True)
            sys.exit(1)                       # a fault or an abort: start nothing more on the device
        res[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(rep, name, json.dumps(res[name][-1]), flush=True)
        if "--out" in sys.argv:
            with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
                json.dump(res, f, indent=1)
