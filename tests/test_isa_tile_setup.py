"""ISA guards of the tile kernels' new-tile path (CPU side: hipcc cross-compiles gfx950 without a GPU; helpers of test_isa_guards.py).

When a wave of the scan kernel (logo_eval_pair_kernel) reaches the end of a band, or a wave of the linear analysis kernel its tile's last
frame, it requests the next tile's logo coefficients a and b and then the next raw samples.  The product b * maxv -- the first use of
the coefficients -- is formed later, where the loads have long landed (eval_tile_stage.h TileStager::coefs_landed, LinStager's
coef_fresh).  Formed at the load it put a wait for two 16-byte loads in front of the raw request and of the whole evaluation that
follows -- a memory round trip per band that every wave of the workgroup reaches at the same time.  So:

  * between a group of coefficient loads (global_load_dwordx4) and the raw-sample request behind it (buffer_load) there is no
    `s_waitcnt vmcnt`, in the prologue and in the loop, in both kernels and for both sample sizes.  (Between the group's FIRST and
    its last load the scheduler may place a wait that belongs to the conversion before them -- the 16-bit scan kernel has one for the
    second unit's raw samples: such a wait is accepted only if its count is too high to cover any of the coefficient loads issued
    so far);
  * the registers stay within the budgets the occupancy plan rests on -- linear <= 128 (four waves per SIMD), pair <= 130 / 136 for
    8-bit / 16-bit samples (three waves per SIMD with room to spare) -- with no scratch;
  * the linear kernel's hand-placed waits still cover every register its inline-assembly loads write.
"""
import re

import pytest

import test_isa_guards as G

BUDGETS = {
    "eval_pair_kernels.hip": {"logo_eval_pair_kernelIhE": 130, "logo_eval_pair_kernelItE": 136},
    "eval_linear_kernels.hip": {"logo_eval_linear_kernel16E": 128, "logo_eval_linear_kernelE": 128},
}


def waits_between_coef_loads_and_raw_request(body):
    """body: instruction lines of one kernel.  Returns (groups found, [offending waits]): a group is a run of >= 4 global_load_dwordx4
    with fewer than 40 lines between neighbours; from its last load to the next buffer_load no vmcnt wait may appear, and a wait
    inside the group must leave every load of the group issued before it outstanding."""
    idx = [i for i, l in enumerate(body) if re.match(r"\s*global_load_dwordx4\b", l)]
    groups, cur = [], []
    for i in idx:
        if cur and i - cur[-1] >= 40:
            groups.append(cur)
            cur = []
        cur.append(i)
    if cur:
        groups.append(cur)
    groups = [g for g in groups if len(g) >= 4]
    hits, found = [], 0
    for g in groups:
        nxt = next((j for j in range(g[-1] + 1, len(body)) if re.match(r"\s*buffer_load_", body[j])), None)
        if nxt is None or nxt - g[-1] > 150:       # (not followed by a raw request: some other use of 16-byte loads)
            continue
        found += 1
        issued = 0                                  # vector-memory loads since the group's first (they return in order)
        for j in range(g[0], nxt):
            t = body[j]
            if re.match(r"\s*(global_load|buffer_load)_", t):
                issued += 1
            w = re.match(r"\s*s_waitcnt\b.*vmcnt\((\d+)\)", t)
            if w and (j > g[-1] or int(w.group(1)) < issued):
                hits.append((j, t.strip()))
    return found, hits


def test_wait_scan_sees_a_planted_wait():
    loads = ["global_load_dwordx4 v[2:5], v6, s[0:1]"] * 4
    good = loads + ["v_add_u32 v1, v2, v3", "buffer_load_dword v9, v1, s[4:7], 0 offen", "s_waitcnt vmcnt(0)"]
    bad = loads + ["s_waitcnt vmcnt(3)", "v_mul_f32 v2, v2, v7", "buffer_load_dword v9, v1, s[4:7], 0 offen"]
    assert waits_between_coef_loads_and_raw_request(good) == (1, [])
    n, hits = waits_between_coef_loads_and_raw_request(bad)
    assert n == 1 and hits
    # inside the group: a wait that cannot reach the group's loads passes, one that can does not
    inside_ok = loads[:2] + ["s_waitcnt vmcnt(4)"] + loads[2:] + ["buffer_load_dword v9, v1, s[4:7], 0 offen"]
    inside_bad = loads[:2] + ["s_waitcnt vmcnt(1)"] + loads[2:] + ["buffer_load_dword v9, v1, s[4:7], 0 offen"]
    assert waits_between_coef_loads_and_raw_request(inside_ok) == (1, [])
    assert waits_between_coef_loads_and_raw_request(inside_bad)[1]


@pytest.mark.parametrize("name", sorted(BUDGETS))
def test_new_tile_path(name):
    asm = G.compile_asm(name)
    ks = G.kernels_of(asm)
    seen = set()
    for kname, k in ks.items():
        sub = next((s for s in BUDGETS[name] if s in kname), None)
        if sub is None:
            continue
        seen.add(sub)
        m = k["meta"]
        print(f"{kname}: {m['vgpr_count']} VGPRs, {m['agpr_count']} AGPRs, scratch {m['private_segment_fixed_size']}")
        assert m["vgpr_count"] + m["agpr_count"] <= BUDGETS[name][sub], f"{kname}: {m['vgpr_count']} VGPRs (+{m['agpr_count']} AGPRs) > {BUDGETS[name][sub]}"
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, f"{kname}: scratch / spills {m}"
        assert not any("scratch_" in l for l in k["body"]), f"{kname}: scratch instructions"
        found, hits = waits_between_coef_loads_and_raw_request(k["body"])
        # the prologue and the loop (the linear kernel: its blended and its field-logo instance, each with both)
        assert found >= 2, f"{kname}: coefficient loads followed by a raw request found {found} times"
        assert not hits, f"{kname}: a vmcnt wait between the coefficient loads and the raw request: {hits[:3]}"
    assert seen == set(BUDGETS[name]), f"kernels not found in {name}: {set(BUDGETS[name]) - seen}"


def test_linear_kernel_in_flight_scan_still_holds():
    asm = G.compile_asm("eval_linear_kernels.hip")
    bodies = {k: v for k, v in G.raw_kernel_bodies(asm).items() if "logo_eval_linear_kernel" in k}
    assert len(bodies) == 2
    for kname, body in bodies.items():
        assert not G.reads_of_registers_in_flight(body), kname
