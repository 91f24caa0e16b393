"""ISA guards of the scan kernel's unscaled staging (CPU side: hipcc cross-compiles gfx950 without a GPU; helpers of test_isa_guards.py
and test_isa_linear_valu.py).

The scan (pair) kernel is limited by the number of vector instructions it issues (profiles/stage_unscaled_notes.md),
so DeintY's `x 0.25` per staged sample is pinned down as gone:

  * logo_eval_pair_kernel stages the [1 2 1] sums unscaled on taps that carry the factor (csrc/eval_tile_stage.h Quad): no v_ldexp_f32
    inside its loop, at either sample size.  The form that scales every sample lives on in a kernel of its own
    (logo_eval_pair_ldexp_kernel) for logos whose taps cannot be scaled: that one still has the eight per loop;
  * the static count of vector instructions of both instances is below the parent commit's (479 / 499 in KERNELS, counted with
    test_isa_linear_valu.v_lines on the commit before this change; the change itself: 471 / 483);
  * registers within the occupancy step the kernels had (128 / 134), no scratch.

(The same staging and a `y - fract(y)` form of the fades' bins were built for the linear analysis kernel as well -- 2994 -> 2976 and
3128 -> 3093 vector instructions -- did not measure faster and were taken out again: profiles/stage_unscaled_notes.md.  That kernel's
guards are tests/test_isa_linear_valu.py, unchanged.)
"""
import re

import test_isa_guards as G
import test_isa_linear_valu as LV

PAIR = "eval_pair_kernels.hip"
# kernel-name substring: (vector instructions on the parent commit, VGPR limit)
KERNELS = {"logo_eval_pair_kernelIhE": (479, 128), "logo_eval_pair_kernelItE": (499, 134)}
LDEXP_FORM = ["logo_eval_pair_ldexp_kernelIhE", "logo_eval_pair_ldexp_kernelItE"]


def count(body, a, b, mnemonic):
    return sum(1 for l in body[a:b + 1] if re.match(rf"\s*{mnemonic}(_e32|_e64|_sdwa|_dpp)?\s", l))


def kernels(subs):
    ks = G.kernels_of(G.compile_asm(PAIR))
    out = {sub: k for kname, k in ks.items() for sub in subs if sub in kname}
    assert set(out) == set(subs), f"kernels not found: {set(subs) - set(out)}"
    return out


def test_counter_sees_planted_instructions():
    body = [".LBB0_1:", "\tv_ldexp_f32 v1, v2, -2", "\tv_ldexp_f32_e64 v3, v4, s2", "\tv_ldexp_f16_e32 v5, v4, v1", "\tbuffer_load_dword v5, v1, s[0:3], 0 offen",
            "\ts_cbranch_scc1 .LBB0_1", "\tv_ldexp_f32 v1, v2, -2"]
    (a, b), = LV.main_loops(body)
    assert count(body, a, b, "v_ldexp_f32") == 2 and count(body, 0, len(body) - 1, "v_ldexp_f32") == 3


def test_no_ldexp_in_the_scan_kernels_loop():
    for sub, k in kernels(KERNELS).items():
        body = k["body"]
        loops = LV.main_loops(body)
        assert len(loops) == 1, (sub, loops)
        (a, b), = loops
        n, ncvt = count(body, a, b, "v_ldexp_f32"), count(body, a, b, "v_cvt_f32_u32")
        print(f"{sub}: loop {a}..{b}: {LV.v_lines(body[a:b + 1])} v_* lines, {n} v_ldexp_f32, {ncvt} v_cvt_f32_u32")
        assert n == 0, f"{sub}: {n} v_ldexp_f32 in the loop"
        assert ncvt == 8, f"{sub}: the staging's conversions are not where they were ({ncvt})"      # (two units of four samples)


def test_the_ldexp_form_lives_on_in_a_kernel_of_its_own():
    for sub, k in kernels(LDEXP_FORM).items():
        body = k["body"]
        (a, b), = LV.main_loops(body)
        n = count(body, a, b, "v_ldexp_f32")
        print(f"{sub}: {n} v_ldexp_f32 in the loop")
        assert n == 8, (sub, n)
        m = k["meta"]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and not any("scratch_" in l for l in body), (sub, m)
        assert m["vgpr_count"] + m["agpr_count"] <= (134 if "ItE" in sub else 128), (sub, m)


def test_fewer_vector_instructions_within_the_same_registers():
    for sub, k in kernels(KERNELS).items():
        parent, vgprs = KERNELS[sub]
        n, m = LV.v_lines(k["body"]), k["meta"]
        print(f"{sub}: {n} v_* lines (parent {parent}), {m['vgpr_count']} VGPRs (limit {vgprs}), scratch {m['private_segment_fixed_size']}")
        assert n < parent, f"{sub}: {n} vector instructions, the parent had {parent}"
        assert m["vgpr_count"] + m["agpr_count"] <= vgprs, f"{sub}: {m['vgpr_count']} VGPRs (+{m['agpr_count']} AGPRs) > {vgprs}"
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and not any("scratch_" in l for l in k["body"]), (sub, m)
