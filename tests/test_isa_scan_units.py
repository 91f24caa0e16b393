"""ISA guards of the scan kernel's one-unit form (CPU side: hipcc cross-compiles gfx950 without a GPU; helpers of test_isa_guards.py,
test_isa_tile_setup.py and test_isa_linear_valu.py).

eval_pair1_kernels.hip instantiates the body of the scan's pair kernel (csrc/eval_pair_body.h) with one staging unit per lane, for
engines whose plans list the units a tile needs (csrc/eval_tiles.hpp kTileCutUnits).  The kernel is bound by the vector instructions it
issues, so what the form is for is pinned down here, against the two-unit form compiled in the same test:

  * no scratch, no vector or scalar spills;
  * VGPRs not above the two-unit form's for the same sample type;
  * in the loop three raw-sample buffer loads per request and, at 8 bits, four sample conversions (one unit of four samples);
  * fewer vector instructions in the loop than the two-unit form;
  * no vmcnt wait between the next tile's coefficient loads and its raw request: the unit word that all of a tile's addresses depend
    on is a register by then, not a load (the walker of test_isa_tile_setup.py);
  * no register is read while a load of it is in flight (the scan of test_isa_guards.py).
"""
import hashlib
import os
import re
import subprocess

import pytest

import test_isa_guards as G
import test_isa_linear_valu as LV
import test_isa_tile_setup as TS

ONE, TWO = "eval_pair1_kernels.hip", "eval_pair_kernels.hip"
# one-unit kernel -> its two-unit partner (Ih: 8-bit samples, It: 16-bit)
PARTNER = {
    "logo_eval_pair1_kernelIhE": "logo_eval_pair_kernelIhE", "logo_eval_pair1_kernelItE": "logo_eval_pair_kernelItE",
    "logo_eval_pair1_ldexp_kernelIhE": "logo_eval_pair_ldexp_kernelIhE", "logo_eval_pair1_ldexp_kernelItE": "logo_eval_pair_ldexp_kernelItE",
}


def compile_asm(name):
    """test_isa_guards.compile_asm for a file that has no entry in its table: build.py's flags, the same cache"""
    from amatsukaze_amd import build as B
    src = os.path.join(G.CSRC, name)
    flags = [f for f in B.FLAGS if f not in ("-fPIC",)] + B.EXTRA_FLAGS.get(name, [])
    deps = [src] + [os.path.join(G.CSRC, f) for f in os.listdir(G.CSRC) if f.endswith((".h", ".hpp"))]
    h = hashlib.sha256(" ".join(flags).encode())
    for d in sorted(deps):
        h.update(open(d, "rb").read())
    os.makedirs(G.CACHE, exist_ok=True)
    out = os.path.join(G.CACHE, f"{name}.{h.hexdigest()[:16]}.s")
    if not os.path.exists(out):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call([B.hipcc()] + flags + ["-S", "--cuda-device-only", "-o", tmp, src], stderr=subprocess.DEVNULL)
        os.replace(tmp, out)
    return open(out).read()


@pytest.fixture(scope="module")
def forms():
    """{one-unit kernel: (its kernels_of entry, its partner's, its raw body)}"""
    asm1 = compile_asm(ONE)
    one, two, raw = G.kernels_of(asm1), G.kernels_of(compile_asm(TWO)), G.raw_kernel_bodies(asm1)
    assert len(one) == 4, sorted(one)
    out = {}
    for sub, psub in PARTNER.items():
        (k1,), (k2,) = [n for n in one if sub in n], [n for n in two if psub in n]
        out[sub] = (one[k1], two[k2], raw[k1])
    return out


def loop_of(body):
    (a, b), = LV.main_loops(body)
    return body[a:b + 1]


def count(lines, pattern):
    return sum(1 for l in lines if re.match(rf"\s*{pattern}", l))


@pytest.mark.parametrize("sub", sorted(PARTNER))
def test_one_unit_form(forms, sub):
    k1, k2, raw = forms[sub]
    m1, m2 = k1["meta"], k2["meta"]
    loop1, loop2 = loop_of(k1["body"]), loop_of(k2["body"])
    v1, v2 = LV.v_lines(loop1), LV.v_lines(loop2)
    loads1, loads2 = count(loop1, r"buffer_load_"), count(loop2, r"buffer_load_")
    cvt1, cvt2 = count(loop1, r"v_cvt_f32_u32"), count(loop2, r"v_cvt_f32_u32")
    print(f"{sub}: {m1['vgpr_count']} VGPRs (two-unit {m2['vgpr_count']}), loop {v1} v_* lines ({v2}), {loads1} raw loads ({loads2}), "
          f"{cvt1} conversions ({cvt2}), {len(loop1)} lines ({len(loop2)})")
    assert m1["private_segment_fixed_size"] == 0 and m1["vgpr_spill_count"] == 0 and m1["sgpr_spill_count"] == 0, m1
    assert not any("scratch_" in l for l in k1["body"])
    assert m1["vgpr_count"] + m1["agpr_count"] <= m2["vgpr_count"] + m2["agpr_count"]
    assert loads1 == 3 and loads2 == 6
    if "Ih" in sub:
        assert cvt1 == 4 and cvt2 == 8
    assert v1 < v2
    found, hits = TS.waits_between_coef_loads_and_raw_request(k1["body"])
    # (two coefficient loads per tile here, below the walker's group size of four: the walk is repeated on pairs below)
    assert not hits, hits[:3]
    found2, hits2 = waits_after_coef_pairs(k1["body"])
    assert found2 >= 2, f"coefficient loads followed by a raw request found {found2} times"      # the prologue and the loop
    assert not hits2, hits2[:3]
    assert not G.reads_of_registers_in_flight(raw)


def waits_after_coef_pairs(body):
    """test_isa_tile_setup's walk for the one-unit form, whose tile has TWO 16-byte coefficient loads (a and b of one unit): from the
    second of two neighbouring global_load_dwordx4 to the next buffer_load no vmcnt wait may appear, and a wait between the two must leave
    the first outstanding"""
    idx = [i for i, l in enumerate(body) if re.match(r"\s*global_load_dwordx4\b", l)]
    pairs = [(a, b) for a, b in zip(idx, idx[1:]) if b - a < 40]
    hits, found = [], 0
    for a, b in pairs:
        nxt = next((j for j in range(b + 1, len(body)) if re.match(r"\s*buffer_load_", body[j])), None)
        if nxt is None or nxt - b > 150:
            continue
        found += 1
        issued = 0
        for j in range(a, nxt):
            t = body[j]
            if re.match(r"\s*(global_load|buffer_load)_", t):
                issued += 1
            w = re.match(r"\s*s_waitcnt\b.*vmcnt\((\d+)\)", t)
            if w and (j > b or int(w.group(1)) < issued):
                hits.append((j, t.strip()))
    return found, hits


def test_pair_walk_sees_a_planted_wait():
    loads = ["global_load_dwordx4 v[2:5], v6, s[0:1]"] * 2
    good = loads + ["v_add_u32 v1, v2, v3", "buffer_load_dword v9, v1, s[4:7], 0 offen", "s_waitcnt vmcnt(0)"]
    bad = loads + ["s_waitcnt vmcnt(1)", "buffer_load_dword v9, v1, s[4:7], 0 offen"]
    assert waits_after_coef_pairs(good) == (1, [])
    assert waits_after_coef_pairs(bad)[1]
