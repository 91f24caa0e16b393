"""The inputs of tests/test_gpu_weave_forms.py and tests/test_gpu_row_copies.py, judged without a GPU: every case of
tests/copy_cases.py reaches the kernel form, the tail and the number of rounds it is listed for, and the numpy weave is the
definition on a picture pair written out by hand.  A case that does not reach its form is not a test of it: fix the case."""
import numpy as np
import pytest

import copy_cases as K


@pytest.mark.parametrize("case", K.WEAVE_CASES, ids=lambda c: c.name)
def test_weave_case_is_what_it_claims(case):
    assert K.weave_form(case) == case.form
    assert K.weave_tails(case) == case.tail
    assert K.weave_rounds(case) == case.rounds
    for w in K.planes_of(case):
        pl = K.plane(case, w)
        assert pl.base >= K.GUARD and pl.base + (pl.frames - 1) * pl.stride + (pl.rows - 1) * pl.pitch + pl.row + K.GUARD <= pl.size
        assert pl.base % case.es == 0 and pl.stride % case.es == 0 and pl.size % 16 == 0


def test_weave_table_reaches_every_branch():
    by = {c.name: c for c in K.WEAVE_CASES}
    vec8 = [c for c in K.WEAVE_CASES if c.form == "vec" and c.es == 1 and not c.nv12]
    # the vector path at one byte per sample: whole rows, an even and an odd partial vector, more than one round with a partial vector
    assert any(c.tail == (0, 0) for c in vec8) and any(c.tail[0] and c.tail[0] % 2 == 0 for c in vec8)
    assert any(c.tail[1] % 2 == 1 for c in vec8) and any(c.rounds[0] >= 3 and c.tail[0] for c in vec8)
    assert by["03-vec-three-rounds"].rounds == (3, 2) and by["03-vec-three-rounds"].tail == (10, 5)
    # two bytes per sample with a partial vector in both kernels; the MSB call at 16 bits shifts by nothing (the plain kernel)
    assert {(c.msb, c.shift) for c in K.WEAVE_CASES if c.form == "vec" and c.es == 2 and any(c.tail)} >= {(False, 0), (True, 4)}
    assert by["14-16bit-msb"].msb and by["14-16bit-msb"].shift == 0
    # the element path for each reason on its own: a pitch, a destination base, a source chroma base, a frame stride
    base = by["01-vec-whole"]
    for name, moved in (("06-elem-by-dstY-base", "dstY"), ("07-elem-by-srcV-base", "srcV"), ("08-elem-by-8-byte-gap", "srcY")):
        c = by[name]
        assert c.form == "elem" and (c.W, c.H, c.bits, c.src_pitch, c.dst_pitch) == (base.W, base.H, base.bits, base.src_pitch, base.dst_pitch)
        bad = [w for w in K.planes_of(c) if (K.plane(c, w).base % 16, K.plane(c, w).stride % 16) != (0, 0)]
        assert bad == [moved]
    assert by["05-elem-by-pitch"].rounds[0] > 1 and by["13-elem-10bit-msb"].rounds[0] > 1          # rows longer than a wave's round
    assert by["09-vec-16-byte-gap"].form == "vec" and K.plane(by["09-vec-16-byte-gap"], "srcY").stride == 12 * 96 + 16
    # NV12: a second round of the split at both sample sizes; a moved interleaved plane leaves the luma on the vector path
    assert all(by[n].nv12 and by[n].rounds[1] == 2 for n in ("10-nv12-two-split-rounds", "12-nv12-10bit", "12-nv12-10bit-msb"))
    assert by["11-nv12-uv-base-moved"].form == "vec" and K.plane(by["11-nv12-uv-base-moved"], "srcU").base % 16 == 2
    # H = 12: the Y / U boundary (row 12) and the U / V boundary (row 18) both fall inside a workgroup of 8 rows
    assert base.H % 8 and (base.H + base.H // 2) % 8 and base.H % 4 == 0


def test_index_arrays_are_what_the_cases_need():
    pairs = list(zip(K.TOP, K.BOTTOM))
    assert len(pairs) == K.N and set(K.TOP) == set(K.BOTTOM) == set(range(K.P))
    assert any(t < b for t, b in pairs) and any(t > b for t, b in pairs) and any(t == b for t, b in pairs)
    assert len(set(K.TOP)) < K.N and len(set(K.BOTTOM)) < K.N


def test_numpy_weave_on_a_hand_written_pair():
    Y = np.array([[[10, 11, 12, 13], [14, 15, 16, 17], [18, 19, 20, 21], [22, 23, 24, 25]],
                  [[50, 51, 52, 53], [54, 55, 56, 57], [58, 59, 60, 61], [62, 63, 64, 65]]], np.uint8)
    U = np.array([[[1, 2], [3, 4]], [[5, 6], [7, 8]]], np.uint8)
    V = U + 100
    dY, dU, dV = K.weave(Y, U, V, [0, 1], [1, 1], False)
    assert dY[0].tolist() == [[10, 11, 12, 13], [54, 55, 56, 57], [18, 19, 20, 21], [62, 63, 64, 65]]
    assert dU[0].tolist() == [[1, 2], [7, 8]] and dV[0].tolist() == [[101, 102], [107, 108]]
    assert np.array_equal(dY[1], Y[1]) and np.array_equal(dU[1], U[1]) and np.array_equal(dV[1], V[1])
    # NV12: U0 V0 U1 V1 in one plane
    UV = np.array([[[1, 101, 2, 102], [3, 103, 4, 104]], [[5, 105, 6, 106], [7, 107, 8, 108]]], np.uint8)
    for got, want in zip(K.weave(Y, UV, None, [0, 1], [1, 1], True), (dY, dU, dV)):
        assert np.array_equal(got, want)
    # MSB containers: the 10-bit sample in the high bits, whatever the low six hold
    m = lambda a: (a.astype(np.uint16) << 6) | 0x2B
    for got, want in zip(K.weave(m(Y), m(U), m(V), [0, 1], [1, 1], False, shift=6), (dY, dU, dV)):
        assert got.dtype == np.uint16 and np.array_equal(got, want)


def test_expected_buffers_keep_the_sentinel_around_the_samples():
    case = next(c for c in K.WEAVE_CASES if c.name == "02-vec-tails")
    src = K.weave_source(case)
    want = K.weave_expected(case, src, None, None, K.P)
    for w, buf in want.items():
        pl = K.plane(case, w)
        s = K.samples(case, w, buf)
        assert np.all(s[K.P:] == K.SENTINEL) and np.all(buf[:pl.base] == K.SENTINEL)              # the sixth frame was not woven
        assert int((buf != K.SENTINEL).sum()) <= K.P * pl.rows * pl.row
    assert np.array_equal(K.samples(case, "dstY", want["dstY"])[3, 0::2], K.samples(case, "srcY", src["srcY"])[3, 0::2])
    # the MSB call at 16 bits expects what the plain call expects
    a, b = (next(c for c in K.WEAVE_CASES if c.name == n) for n in ("14-16bit", "14-16bit-msb"))
    sa, sb = K.weave_source(a), K.weave_source(b)
    assert all(np.array_equal(sa[w], sb[w]) for w in sa)
    wa, wb = K.weave_expected(a, sa, K.TOP, K.BOTTOM, K.N), K.weave_expected(b, sb, K.TOP, K.BOTTOM, K.N)
    assert all(np.array_equal(wa[w], wb[w]) for w in wa)


@pytest.mark.parametrize("case", K.WEAVE_CASES, ids=lambda c: c.name)
def test_expected_buffers_are_what_the_oracle_writes(case):
    """orc_merge_field (the C restatement of MergeField) frame by frame into the same flat buffers; MSB pictures shifted beforehand"""
    from amtlib import Oracle
    orc = Oracle()
    src = K.weave_source(case)
    lsb = {w: (b.view("<u2") >> case.shift).view(np.uint8) if case.shift else b for w, b in src.items()}
    L = {w: K.plane(case, w) for w in K.planes_of(case)}
    got = {w: K.blank(case, w) for w in K.PLANES[3:]}
    at = lambda bufs, w, i: bufs[w].ctypes.data + L[w].base + i * L[w].stride if w in bufs else None
    for i, (t, b) in enumerate(zip(K.TOP, K.BOTTOM)):
        orc.lib.orc_merge_field(at(lsb, "srcY", t), at(lsb, "srcU", t), at(lsb, "srcV", t), at(lsb, "srcY", b), at(lsb, "srcU", b),
                                at(lsb, "srcV", b), case.src_pitch[0], case.src_pitch[1], int(case.nv12), case.bits, case.W, case.H,
                                at(got, "dstY", i), at(got, "dstU", i), at(got, "dstV", i), case.dst_pitch[0], case.dst_pitch[1])
    want = K.weave_expected(case, src, K.TOP, K.BOTTOM, K.N)
    for w in want:
        assert not K.first_difference(got[w], want[w]), w


def test_row_tables_reach_every_lane_width():
    for c in K.STRIDED_UPLOADS + [K.TWO_SLOT_STRIDED, K.TWO_SLOT_GATHER] + K.SMALL_GATHERS:
        im = K.image(c.chunk, c.pitch, c.off, c.nchunks)
        assert (im.base - c.off) % 16 == 0 and im.size % 16 == 0
        assert K.row_lanes(0, c.chunk, im.base, c.pitch, c.chunk) == c.lanes, c.id
        assert c.pitch > c.chunk                                   # (rows as wide as the pitch leave by the copy engine, not the kernel)
        assert (c.chunk // c.lanes * c.nchunks) % 256 != 0, c.id   # the last workgroup is partly idle
    assert [c.lanes for c in K.STRIDED_UPLOADS] == [16, 4, 1, 4, 1, 1, 16, 1]
    passes = [c.chunk // c.lanes * c.nchunks > K.GRID_PASS for c in K.STRIDED_UPLOADS]
    assert passes == [False] * 7 + [True] and K.STRIDED_UPLOADS[-1].lanes == 1
    assert K.STRIDED_UPLOADS[6].nchunks == 1
    # the download reads the device image and writes packed chunks
    assert [K.row_lanes(K.image(c.chunk, c.pitch, c.off, c.nchunks).base, c.pitch, 0, c.chunk, c.chunk) for c in K.DOWNLOADS] == [16, 4, 1]
    # the registered pool
    c = K.POOL_CASE
    assert c.lanes == 16
    for (off, stride), lanes in K.POOL_SOURCES.items():
        assert K.row_lanes(off, stride, K.image(c.chunk, c.pitch, c.off, c.nchunks).base, c.pitch, c.chunk) == lanes
    assert sorted(set(K.POOL_SOURCES.values())) == [1, 4, 16] and {o for o, s in K.POOL_SOURCES} == {0, 4, 1}


def test_two_slot_cases_cut_where_they_claim():
    s, g = K.TWO_SLOT_STRIDED, K.TWO_SLOT_GATHER
    assert (s.chunk, s.pitch, s.nchunks) == ((5 << 20) + 4, (5 << 20) + 4 + 12, 8)
    per_slot = K.SLOT_BYTES // s.chunk
    assert 0 < per_slot < s.nchunks <= 2 * per_slot                # the second launch writes from chunk `per_slot` on
    assert g.chunk == (3 << 20) + 4 and g.nchunks == K.GATHER_SOURCES * K.GATHER_CHUNKS_PER_SOURCE == 12
    cut = K.SLOT_BYTES // g.chunk
    assert cut < g.nchunks <= 2 * cut
    assert cut // K.GATHER_CHUNKS_PER_SOURCE == 2 and cut % K.GATHER_CHUNKS_PER_SOURCE != 0      # inside the third source
    assert all(c.nchunks % 5 == 0 for c in K.SMALL_GATHERS)
