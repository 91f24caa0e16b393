"""The cadence renderer's adaptive bob (kfm_render(..., deint="adaptive"), csrc/render_adaptive_kernels.hip) measured on an MI355X
beside the line rule; writes profiles/kfm_render_adaptive.json.

  1920x1080 at 8 and at 10 bits, 1 024 source frames resident in HBM (3.2 / 6.4 GB; with the destination far above the 256 MiB Infinity
  Cache), an all-60i plan (2 048 bobbed fields).  Three rules alternate in the same run on the same buffers: the adaptive rule, the line
  rule with thresh -1 and the line rule with thresh 4.  Times are the context's HIP events around the one kernel launch of a call
  (Context.profile), median [min - max] of 7 after 2 warm-up calls.

  Algorithmic bytes of a bobbed field of F bytes under the adaptive rule: frame n whole (F: kept rows, U / D, and the missing parity as
  A or B), one neighbour whole (F: its rows y -+ 1 for the motion test, its missing-parity rows as A or B), the other neighbour's
  kept-parity rows (F / 2, the motion test), plus F written = 3.5 F + F; at a clip end one neighbour is frame n itself: 2.5 F + F.  The
  line rule's bytes are tools/kfm_render_bench.py's.  The kernel ISSUES more loads than that (a source row is read by up to five output
  rows); what of that reaches HBM is not measured here.

  From the ISA (the file compiled as build.py compiles it): the vector instructions in the loop that interpolates one 16-byte span per
  lane.  With them, a lower bound of the arithmetic's time: spans / 64 lanes wave-instructions, each 4 cycles of a SIMD's 16 lanes wide
  vector unit (packed 16-bit and plain 32-bit integer operations alike; dual-issue and the scalar unit not counted), over 256 CUs x 4
  SIMDs at 2.4 GHz -- to say which of the two bounds, memory or arithmetic, the kernel runs against.

  Outputs at the timed size are checked against the numpy restatement (tests/kfm_render_adaptive_ref.py) on a sample of rows of the
  first, the last and two middle fields before any timing.

    python tools/kfm_render_adaptive_bench.py [--out profiles/kfm_render_adaptive.json] [--frames 1024]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kfm_render_bench import H, HBM_PEAK, REPS, THRESH, W, WARMUP, algorithmic_bytes, clip, kernel_ms, rates, spread  # noqa: E402

CUS, SIMDS_PER_CU, CLOCK_HZ, CYCLES_PER_WAVE_VALU = 256, 4, 2.4e9, 4
SAMPLE_ROWS = 12


def adaptive_bytes(plan, frame_bytes, clip_frames):
    return sum((3.5 if (top == 0 or top == clip_frames - 1) else 4.5) * frame_bytes for _, top, _, _ in plan)


def span_loop_isa():
    """{form: vector instructions (and all instructions) in the loop that holds the 12 loads of a span}, from hipcc's assembly"""
    from amatsukaze_amd import build as B
    name = "render_adaptive_kernels.hip"
    flags = [f for f in B.FLAGS if f != "-fPIC"] + B.EXTRA_FLAGS.get(name, [])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.check_call([B.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(B.CSRC, name)], stderr=subprocess.DEVNULL)
        asm = open(out).read()
    res = {}
    for tag, form in (("ILi1ELb1E", "8-bit containers, 16 bytes per lane"), ("ILi2ELb1E", "16-bit containers, 16 bytes per lane")):
        m = re.search(r"^(_ZN3amt26kfm_render_adaptive_kernel%s\w*):[^\n]*\n(.*?)^\.Lfunc_end" % tag, asm, re.M | re.S)
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
        header = next(lbl for lbl, loop, ins in blocks if sum(i.startswith("global_load_dwordx4") for i in ins) >= 12)
        body = [i for lbl, loop, ins in blocks if loop == header for i in ins]
        res[form] = {"vector_instructions_per_span": sum(i.startswith("v_") for i in body), "instructions_per_span": len(body),
                     "packed_16_bit": sum(i.startswith("v_pk_") for i in body), "dpp_moves": sum("_dpp" in i for i in body),
                     "loads_16_bytes": sum(i.startswith("global_load_dwordx4") for i in body),
                     "container_loads_on_seam_lanes": sum(bool(re.match(r"global_load_(ubyte|ushort)", i)) for i in body)}
    return res


def check_rows(np, A, src, dst, plan, bits):
    """SAMPLE_ROWS missing rows (both plane kinds, the plane's first and last row among them) of the first two, two middle and the last
    two fields against the numpy restatement; returns the rows checked"""
    dt = np.uint8 if bits <= 8 else np.uint16
    host = lambda t: t.cpu().numpy().view(dt)
    n, rows = src.num_frames, 0
    for k in (0, 1, len(plan) // 2, len(plan) // 2 + 1, len(plan) - 2, len(plan) - 1):
        kind, f = int(plan[k]["kind"]), int(plan[k]["top"])
        lo, hi = max(0, f - 1), min(n - 1, f + 1)
        for s, d in ((src.Y, dst.Y), (src.U, dst.U), (src.V, dst.V)):
            C, P, N, got = host(s[f]), host(s[lo]), host(s[hi]), host(d[k])
            Aa, Bb = (P, C) if kind == 1 else (C, N)
            h = C.shape[0]
            missing = list(range(1 if kind == 1 else 0, h, 2))
            for y in sorted(set(missing[:2] + missing[-2:] + missing[::max(1, len(missing) // (SAMPLE_ROWS - 4))])):
                want = A.adaptive_row(C, P, N, Aa, Bb, y)[0]
                assert np.array_equal(got[y], want.astype(dt)), ("output field", k, "row", y)
                rows += 1
            kept = slice(0 if kind == 1 else 1, h, 2)
            assert np.array_equal(got[kept], C[kept]), ("output field", k, "kept rows")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfm_render_adaptive.json"))
    ap.add_argument("--frames", type=int, default=1024)
    args = ap.parse_args()
    import numpy as np
    import torch
    import amatsukaze_amd as A
    import kfm_render_adaptive_ref as RA
    N = args.frames
    isa = span_loop_isa()
    ctx = A.Context(0)
    ctx.profile(True)
    res = {"what": "kfm_render_adaptive_kernel beside kfm_render_kernel, %dx%d, %d source frames in HBM, all-60i plan; HIP events around the launch, "
                   "median [min - max] of %d after %d warm-up calls, the three rules alternating on the same buffers; bytes are algorithmic "
                   "(tools/kfm_render_adaptive_bench.py)" % (W, H, N, REPS, WARMUP),
           "device": torch.cuda.get_device_name(0), "peak_TB_per_s": 8.0, "isa": isa, "cases": []}
    plan = A.kfm_render_plan([0] * N, [0] * N)
    entries = [tuple(int(v) for v in e) for e in plan]
    for bits in (8, 10):
        es = 1 if bits <= 8 else 2
        frame_bytes = (W * H + 2 * (W // 2) * (H // 2)) * es
        src = clip(A, torch, N, bits, seed=77 + bits)
        dst = clip(A, torch, len(plan), bits)
        rules = {
            "adaptive": ("kfm_render_adaptive_kernel", lambda: A.kfm_render(ctx, src, plan, dst, deint="adaptive"), adaptive_bytes(entries, frame_bytes, N)),
            "line, thresh -1": ("kfm_render_kernel", lambda: A.kfm_render(ctx, src, plan, dst, thresh=-1), algorithmic_bytes(entries, frame_bytes, -1, N)),
            "line, thresh %d" % THRESH: ("kfm_render_kernel", lambda: A.kfm_render(ctx, src, plan, dst, thresh=THRESH), algorithmic_bytes(entries, frame_bytes, THRESH, N)),
        }
        rules["adaptive"][1]()
        checked = check_rows(np, RA, src, dst, plan, bits)
        ms = {name: [] for name in rules}
        for i in range(WARMUP + REPS):
            for name, (kernel, call, _) in rules.items():
                t = kernel_ms(ctx, kernel, call)
                if i >= WARMUP:
                    ms[name].append(t)
        for name, (kernel, _, nbytes) in rules.items():
            t = spread(ms[name])
            case = {"rule": name, "kernel": kernel, "bits": bits, "source_frames": N, "output_frames": len(plan), "algorithmic_bytes": nbytes, "ms": t,
                    **rates(nbytes, t)}
            if name == "adaptive":
                form = "%d-bit containers, 16 bytes per lane" % (8 * es)
                spans = len(plan) * (frame_bytes / 2) / 16                # half of a field's rows are interpolated
                valu_ms = spans / 64 * isa[form]["vector_instructions_per_span"] * CYCLES_PER_WAVE_VALU / (CUS * SIMDS_PER_CU * CLOCK_HZ) * 1e3
                mem_ms = nbytes / HBM_PEAK * 1e3
                case.update({"rows_checked_against_numpy": checked, "interpolated_16_byte_spans": spans,
                             "vector_instructions_per_span": isa[form]["vector_instructions_per_span"],
                             "arithmetic_lower_bound_ms": valu_ms, "memory_lower_bound_ms_at_8TBps": mem_ms,
                             "measured_over_arithmetic_bound": t["median"] / valu_ms, "measured_over_memory_bound": t["median"] / mem_ms,
                             "nearer_bound": "arithmetic" if valu_ms > mem_ms else "memory"})
            res["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
        del src, dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
