"""The far-stride layout of tests/far_stride_clips.py, pinned without a GPU and without the gigabytes: addresses, the three frames and the
decoys.  Every window a modelled mutant addresses lies inside the allocation (the safety property of tests/test_gpu_far_strides.py: a
kernel that is wrong in a modelled way shows wrong bytes, it does not fault), overlaps no true frame, and -- for every operation of the GPU
tests -- holds a picture that changes the CPU reference's answer when it is read for the true one."""
import numpy as np
import pytest

import far_stride_clips as F


def test_allocation_under_the_cap():
    assert F.A <= F.CAP and F.A - 12 * F.GiB < 64 * F.MiB
    assert F.D1 % 256 == 0 and F.D2 % 256 == 0 and min(F.D1, F.D2) > len(F.MAIN) * F.SLOT
    assert all(F.window_extent(s) + 2 * F.GUARD <= F.SLOT for s in F.SLOT_NAMES)          # a guard band on both sides of every window
    assert F.A % 2 == 0 and all(F.slot_base(s) % 256 == 0 for s in F.SLOT_NAMES)
    assert max(hi for _, hi, _, _ in F.all_windows()) + F.GUARD <= F.A < max(hi for _, hi, _, _ in F.all_windows()) + F.SLOT


def test_products_cross_the_32_bit_edges():
    """what the two layouts are for: byte offsets past 2^31 and 2^32 (L31), sample offsets of 16-bit planes past 2^31 and 2^32 (L32)"""
    b = [n * F.LAYOUTS["L31"] for n in (1, 2)]
    assert (1 << 31) <= b[0] < (1 << 32) <= b[1]
    s = [n * F.LAYOUTS["L32"] // 2 for n in (1, 2)]
    assert (1 << 31) <= s[0] < (1 << 32) <= s[1]


@pytest.mark.parametrize("layout", F.STRIDES)
@pytest.mark.parametrize("mutant,unit", F.modelled())
def test_mutant_windows_in_bounds_and_off_the_true_frames(layout, mutant, unit):
    Sb = F.STRIDES[layout]
    true = [w for w in F.all_windows() if w[3] == "true"]
    for slot in F.SLOT_NAMES:
        if layout not in F.slot_layouts(slot):
            continue
        ext = F.window_extent(slot)
        for n in range(F.N):
            off = F.mutant_offset(mutant, n, Sb, unit)
            a, b = F.slot_base(slot) + off, F.slot_base(slot) + off + ext
            assert 0 <= a - F.GUARD and b + F.GUARD <= F.A, (slot, n, a, b)                 # (the guard bands the GPU tests read, too)
            if off == F.true_offset(n, Sb):
                continue
            assert (off, n, layout) in F.DECOYS and a in [x for _, x in F.decoy_windows(slot)]     # a decoy of frame n lies there
            for ta, tb, tslot, _ in true:
                assert b <= ta or tb <= a, (slot, n, "overlaps a true window of", tslot)


def test_windows_in_bounds_and_disjoint():
    wins = sorted(F.all_windows())
    assert wins[0][0] - F.GUARD >= 0 and wins[-1][1] + F.GUARD <= F.A
    assert all(a[1] + F.GUARD <= b[0] for a, b in zip(wins, wins[1:])), "a window, true or decoy, touches another or its band"
    assert not [w for w in F.DECOYS if w[2] == "near"]                                      # (near frames: no offset to get wrong)


def test_render_batches_do_not_interleave():
    """what the cadence renderer asks of its two batches: the byte range of every plane of one clear of every plane of the other"""
    def span(slots, layout):
        return (min(F.true_windows(s, layout)[0] for s in slots), max(F.true_windows(s, layout)[-1] + F.window_extent(s) for s in slots))
    main_src, main_dst = ("p8Y", "p8U", "p8V", "p10Y", "p10U", "p10V", "nv12", "p010"), ("dstY", "dstU", "dstV", "dstS")
    rd, near = ("rdY", "rdU", "rdV", "rdS"), ("nearY", "nearU", "nearV", "nearS")
    assert span(main_src, "L31")[1] <= span(rd, "L31")[0]
    assert span(near, "near")[1] <= span(main_src, "L32")[0] and span(near, "near")[1] <= span(main_dst, "L32")[0]
    # and why an L32 batch gets a near partner: two of them do not fit
    assert 2 * (2 * F.LAYOUTS["L32"]) + F.B > F.CAP


def test_every_modelled_mutant_applies_somewhere():
    applies = {(m, u): [(lay, n) for lay, Sb in F.LAYOUTS.items() for n in range(1, F.N)
                        if F.mutant_offset(m, n, Sb, u) != F.true_offset(n, Sb)] for m, u in F.modelled()}
    assert {k for k, v in applies.items() if not v} == F.INERT                               # (the pairs that apply in neither layout)
    # what each layout is there for
    assert {lay for lay, _ in applies[("stride_u32", 1)]} == {"L32"} and {lay for lay, _ in applies[("u32", 2)]} == {"L32"}
    assert ("L31", 1) in applies[("s32", 1)] and ("L31", 2) in applies[("u32", 1)] and ("L32", 1) in applies[("s32", 2)]
    assert len(F.DECOYS) == 6 and {n for _, n, _ in F.DECOYS} == {1, 2}


def test_the_dropped_mutant_would_leave_the_allocation():
    """stride_s32 in samples: frame 2 of L32 lies in front of the allocation whatever the slot, and B cannot grow under the cap"""
    assert list(F.DROPPED) == [("stride_s32", 2)]
    off = F.mutant_offset("stride_s32", 2, F.LAYOUTS["L32"], 2)
    assert F.B + off < 0 and -off - F.B + F.A > F.CAP
    assert all(F.mutant_offset("stride_s32", n, F.LAYOUTS["L31"], 2) == F.true_offset(n, F.LAYOUTS["L31"]) for n in range(F.N))


def test_audio_windows():
    assert F.PCM_ELEM >= 1 << 31 and 2 * F.PCM_ELEM >= 1 << 32 and F.PCM_ELEM % F.CHANNELS == 0 and F.PCM_FIRST >= 0
    assert F.PCM_BASE + 2 * F.PCM_NUMEL <= F.A
    video = [(lo - F.GUARD, hi + F.GUARD) for lo, hi, _, _ in F.all_windows()]
    wins = [F.PCM_TRUE] + list(F.PCM_DECOYS.values())
    assert len(set(wins)) == 3
    for a in wins:
        assert 0 <= a and a + F.PCM_BYTES <= F.A
        assert all(a + F.PCM_BYTES <= va or vb <= a for va, vb in video)
    true, decoy = F.pcm(1), F.pcm(2)
    assert not np.array_equal(F.audio_ref(true), F.audio_ref(decoy))
    assert (F.audio_ref(true)[:, 3] > 0).all()                                               # every video frame owns samples


def test_pictures():
    p = F.pictures()
    for kind in F.KINDS:
        t = p[kind]["true"]
        assert t["Y"].shape == (F.N, F.H, F.W) and len(p[kind]["decoy"]) == len(F.DECOYS)
        assert t["Y"].dtype == (np.uint8 if F.BITS[kind] == 8 else np.uint16)
    assert p["p10"]["true"]["Y"].max() <= 1023 < F.HOT[3]
    assert (p["p010"]["true"]["Y"] & 63).all()                                               # random non-zero low bits under every sample
    f, y, x, _ = F.HOT
    assert f == 2 and F.IMGY <= y < F.IMGY + F.LH and F.IMGX <= x < F.IMGX + F.LW


@pytest.fixture(scope="module")
def refs():
    return F.Refs()


@pytest.fixture(scope="module")
def ops(refs, tmp_path_factory):
    return F.operations(refs, str(tmp_path_factory.mktemp("far")))


def test_every_frame_is_accepted_by_the_scan(refs):
    """LogoScan::AddFrame keeps all three frames (and every decoy in their place): the sums are sums over the frames a kernel read"""
    for w in [None] + list(range(len(F.DECOYS))):
        planes = F.pictures()["p8"]["true"] if w is None else F.swapped("p8", w)
        assert refs.logoscan(planes)[0].tolist() == [1] * F.N


def test_a_wrong_read_changes_the_answer(ops):
    """for every operation and every decoy window: the reference over the frames with the decoy in the true frame's place differs from
    the reference over the true frames in EVERY array the GPU test compares (a decoy replaces all planes of its frame, and every output
    plane is made from its own input plane: a kernel that misplaces one plane only still shows)"""
    pics = F.pictures()
    names = [name for name, _, _ in ops]
    assert len(set(names)) == len(names)
    for name, kind, f in ops:
        want = f(pics[kind]["true"])
        for w in range(len(F.DECOYS)):
            got = f(F.swapped(kind, w))
            assert len(got) == len(want)
            assert all(not np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True) for a, b in zip(got, want)), (name, "decoy", w)


def test_hot_sample_record_is_its_own(refs):
    """the sample above maxv changes frame 2's exact record: the guarded modes must hand that frame to the exact kernel to match it"""
    p10 = F.pictures()["p10"]["true"]
    a, b = refs.analyze(p10, 10), refs.analyze(F.with_hot_sample(p10), 10)
    assert a[:2].tobytes() == b[:2].tobytes() and a[2].tobytes() != b[2].tobytes()
