"""ISA guards of the vector work the tile kernels no longer do (CPU side: hipcc cross-compiles gfx950 without a GPU; helpers of
test_isa_guards.py, budgets of test_isa_tile_setup.py).

The linear analysis kernel is limited by the issue rate of its vector pipe (profiles/linear_valu_notes.md), so what it issues for nothing
is pinned down here:

  * max(|resp|, floorResp) of a term's scale is ONE v_max_f32.  Written with the compiler's builtins it was three: `resp` comes out of
    inline assembly and floorResp out of memory, the compiler cannot know them canonical and puts `v_max_f32 x, |r|, |r|` and
    `v_max_f32 l, L, L` in front -- twelve self-max per trip round the loop.  None may be left inside the loops; outside them (the listed
    pairs' corrections after the loop, once per loop instance) at most two per kernel;
  * the static count of vector instructions of both linear kernels stays below what it was before that change (PARENT_V_LINES: counted
    with v_lines() below on the commit before it);
  * the new-tile path -- from the fetch of a tile's descriptor to the raw-sample request behind it, in the prologue and in the loop of the
    four linear loop instances and of the two scan (pair) kernels -- forms its offsets with 24-bit multiplies (eval_tiles.hpp mul24;
    operand limits enforced on the host, tests/test_tile_mul24.py): no full-width v_mul_lo_u32, which issues at a quarter of the rate.
    No full multiply had to stay on that path.  (The ones left in these kernels multiply 64-bit frame offsets of the listed pairs' exact
    means and the summing wave's row addresses: outside the loops' new-tile path.)
"""
import re

import pytest

import test_isa_guards as G
import test_isa_tile_setup as TS

LINEAR = "eval_linear_kernels.hip"
PAIR = "eval_pair_kernels.hip"
# `^\s+v_` lines of the kernel bodies on the parent commit of the change (v_lines() of this file)
PARENT_V_LINES = {"logo_eval_linear_kernelE": 3032, "logo_eval_linear_kernel16E": 3162}


def v_lines(body):
    return sum(1 for l in body if re.match(r"\s+v_", l))


def self_max(line):
    """v_max_f32 with two identical sources (modifiers included): a canonicalisation"""
    m = re.match(r"\s*v_max_f32\S*\s+v\d+\s*,\s*([^,]+?)\s*,\s*([^,]+?)\s*$", line)
    return bool(m) and m.group(1) == m.group(2)


def main_loops(body):
    """[(first, last)] line ranges of the loops that hold a raw-sample request (buffer_load): label .. the backward branch to it, the
    outermost range per request"""
    lines = [l.strip() for l in body]
    labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            a = labels[m.group(1)]
            if any(x.startswith("buffer_load_") for x in lines[a:i]):
                loops.append((a, i))
    loops.sort()
    out = []
    for a, b in loops:                         # merge nested / overlapping ranges
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def new_tile_paths(body):
    """[(fetch, request)]: from the scalar load of a tile descriptor's `rcp` (s_load_dword at byte 24 -- the field only the staging
    units' setup reads) to the next buffer_load"""
    lines = [l.strip() for l in body]
    out = []
    for i, l in enumerate(lines):
        if re.match(r"s_load_dword\s+s\d+\s*,.*\b0x18$", l):
            nxt = next((j for j in range(i + 1, min(len(lines), i + 400)) if lines[j].startswith("buffer_load_")), None)
            if nxt is not None:
                out.append((i, nxt))
    return out


def test_scans_see_planted_instructions():
    assert self_max("\tv_max_f32_e64 v5, |v3|, |v3|") and self_max("\tv_max_f32_e64 v63, s49, s49") and self_max("\tv_max_f32_e32 v1, v2, v2")
    assert not self_max("\tv_max_f32_e64 v5, |v3|, s49") and not self_max("\tv_max_f32_e32 v1, v2, v3") and not self_max("\tv_max_f32_e64 v5, |v3|, v3")
    loop = [".LBB0_1:", "\tv_max_f32_e32 v1, v2, v2", "\tbuffer_load_dword v5, v1, s[0:3], 0 offen", "\ts_cbranch_scc1 .LBB0_1", "\tv_max_f32_e32 v1, v2, v2"]
    assert main_loops(loop) == [(0, 3)]
    assert main_loops([".LBB0_1:", "\tv_add_f32_e32 v1, v2, v2", "\ts_cbranch_scc1 .LBB0_1"]) == []
    path = ["\ts_load_dwordx4 s[4:7], s[2:3], 0x0", "\ts_load_dword s8, s[2:3], 0x18", "\tv_mul_lo_u32 v1, v2, s8", "\tbuffer_load_dword v5, v1, s[0:3], 0 offen"]
    assert new_tile_paths(path) == [(1, 3)]
    assert new_tile_paths(["\ts_load_dwordx2 s[8:9], s[2:3], 0x18", "\tbuffer_load_dword v5, v1, s[0:3], 0 offen"]) == []
    assert v_lines(["\tv_add_f32_e32 v1, v2, v2", "\ts_nop 0", ".LBB0_1:", "\tv_mov_b32_e32 v1, 0"]) == 2


def linear_kernels():
    ks = G.kernels_of(G.compile_asm(LINEAR))
    out = {sub: k for kname, k in ks.items() for sub in PARENT_V_LINES if sub in kname}
    assert set(out) == set(PARENT_V_LINES)
    return out


def test_no_canonicalising_max_in_the_linear_loops():
    for sub, k in linear_kernels().items():
        body = k["body"]
        loops = main_loops(body)
        assert len(loops) == 2, f"{sub}: the blended and the field-logo loop, found {loops}"
        inside = [(i, body[i].strip()) for a, b in loops for i in range(a, b + 1) if self_max(body[i])]
        outside = [i for i, l in enumerate(body) if self_max(l) and not any(a <= i <= b for a, b in loops)]
        print(f"{sub}: loops {loops}, self-max inside {len(inside)}, outside {len(outside)}")
        assert not inside, f"{sub}: v_max_f32 of a value with itself inside a loop: {inside[:3]}"
        assert len(outside) <= 2, f"{sub}: {len(outside)} canonicalising v_max_f32 outside the loops"
        for a, b in loops:                      # the one-instruction maximum is there: eleven per trip, |resp| against a scalar register
            n = sum(1 for l in body[a:b + 1] if re.match(r"\s*v_max_f32\S*\s+v\d+, \|v\d+\|, s\d+\s*$", l))
            assert n == 11, f"{sub}: {n} v_max_f32 v, |v|, s in the loop at {a}"


def test_linear_kernels_issue_fewer_vector_instructions_than_before():
    for sub, k in linear_kernels().items():
        n = v_lines(k["body"])
        print(f"{sub}: {n} v_* lines (parent {PARENT_V_LINES[sub]})")
        assert n < PARENT_V_LINES[sub], f"{sub}: {n} vector instructions, the parent had {PARENT_V_LINES[sub]}"


@pytest.mark.parametrize("name", [LINEAR, PAIR])
def test_no_full_multiply_on_the_new_tile_path(name):
    ks = {kname: k for kname, k in G.kernels_of(G.compile_asm(name)).items() if any(s in kname for s in TS.BUDGETS[name])}
    assert len(ks) == 2
    for kname, k in ks.items():
        body = k["body"]
        paths = new_tile_paths(body)
        loops = main_loops(body)
        in_loop = [p for p in paths if any(a <= p[0] and p[1] <= b for a, b in loops)]
        print(f"{kname}: new-tile paths {paths}, of them in a loop {in_loop}")
        # every loop instance has one (linear: two instances per kernel; pair: one), and the prologues theirs
        assert len(in_loop) == len(loops) == (2 if name == LINEAR else 1), f"{kname}: {in_loop} / {loops}"
        assert len(paths) > len(in_loop)
        for a, b in paths:
            hits = [(i, body[i].strip()) for i in range(a, b) if re.match(r"\s*v_mul_(lo|hi)_[ui]32\b", body[i])]
            assert not hits, f"{kname}: full-width multiply between the tile fetch at {a} and the raw request at {b}: {hits[:4]}"
            assert any(re.match(r"\s*v_(mul|mad)_u32_u24", body[i]) for i in range(a, b)), f"{kname}: no 24-bit multiply on the path at {a}"


@pytest.mark.parametrize("name", [LINEAR, PAIR])
def test_register_and_scratch_budgets_still_hold(name):
    ks = G.kernels_of(G.compile_asm(name))
    seen = set()
    for kname, k in ks.items():
        sub = next((s for s in TS.BUDGETS[name] if s in kname), None)
        if sub is None:
            continue
        seen.add(sub)
        m = k["meta"]
        assert m["vgpr_count"] + m["agpr_count"] <= TS.BUDGETS[name][sub], (kname, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and not any("scratch_" in l for l in k["body"]), (kname, m)
    assert seen == set(TS.BUDGETS[name])
