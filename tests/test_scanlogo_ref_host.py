"""The CPU reference of the high-bit ScanLogo tests (tests/scanlogo_ref.py), on the CPU: at 8 bits its composition is the oracle's
ScanLogo byte for byte; at 10 and 12 bits it makes a logo from every clip test_gpu_scanlogo_hibit.py uses, with both sides of the
frame-selection rule `minFade > 8` live in each round (0 < re-accumulated < kept)."""
import ctypes as C

import numpy as np
import pytest

import logofind_ref as LF
import scanlogo_hibit_clips as K
import scanlogo_ref as R
from amtlib import Oracle, _ptr


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def refdir(tmp_path_factory):
    return tmp_path_factory.mktemp("scanlogo_ref")


def test_composition_is_the_oracles_scanlogo_at_8_bits(orc, refdir):
    W, H, lw, lh, x, y, n = K.geometry("A")
    clip = K.clip("A", 8)
    Y, U, V = clip["Y"], clip["U"], clip["V"]
    nvalid, nread = C.c_int(), C.c_int()
    lo = orc.lib.orc_scanlogo_mt(_ptr(Y), _ptr(U), _ptr(V), Y.strides[0], U.strides[0], Y.shape[2], U.shape[2], W, H, n, x, y, lw, lh,
                                 K.THY, K.QUOTA, 1, C.byref(nvalid), None, 1, C.byref(nread))
    assert lo
    path = refdir / "orc8.lgd"
    assert orc.lib.orc_logo_save(lo, str(path).encode(), b"No Name", K.SID) == 1
    orc.lib.orc_logo_free(lo)
    got, info = K.reference(orc, "A", 8, refdir)
    print("8 bits:", {k: v for k, v in info.items() if k != "data"})
    assert (info["kept"], info["nread"]) == (nvalid.value, nread.value) == (25, 43)
    assert got == path.read_bytes()


@pytest.mark.parametrize("name,bits,kept,nread,rounds", [
    ("A", 10, 25, 43, [3, 10]),
    ("A", 12, 25, 43, [2, 10]),
    ("odd", 10, 25, 43, [3, 10]),
    ("odd", 12, 25, 43, [3, 10]),
    ("grow", 10, 300, 300, [61, 105]),
])
def test_reference_makes_a_logo_with_both_sides_of_the_selection_live(orc, refdir, name, bits, kept, nread, rounds):
    quota = 1 << 30 if name == "grow" else K.QUOTA
    lgd, info = K.reference(orc, name, bits, refdir, quota=quota)
    print(name, bits, {k: v for k, v in info.items() if k != "data"})
    assert lgd is not None
    assert (info["kept"], info["nread"]) == (kept, nread)
    assert all(0 < r < info["kept"] for r in info["rounds"]) and len(info["rounds"]) == 2
    assert info["rounds"] == rounds


def test_auto_clip_rectangle_and_reference(orc, refdir):
    """the finder's first candidate is the same rectangle at 8, 10 and 12 bits (host ranking over the numpy sums), and the reference makes
    a logo on it at 10 bits"""
    from amatsukaze_amd.api import logo_candidates_host
    W, H, lw, lh, x, y, n = K.geometry("auto")
    for bits in (8, 10, 12):
        cands, total = logo_candidates_host(LF.sums(K.clip("auto", bits)["Y"], W, H), W, H, bits, n, cap=4)
        assert total >= 1
        c = cands[0]
        assert (c.imgx, c.imgy, c.w, c.h) == K.AUTO_RECT, (bits, c)
    lgd, info = K.reference(orc, "auto", 10, refdir, rect=K.AUTO_RECT)
    print("auto 10:", {k: v for k, v in info.items() if k != "data"})
    assert lgd is not None
    assert (info["kept"], info["nread"], info["rounds"]) == (25, 94, [7, 11])
