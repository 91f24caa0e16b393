"""Numpy restatement of the resize on decoder surfaces (amtgpu_resize_run_surfaces, include/amt_gpu.h; DESIGN.md section 6e, "surfaces in
kind"), written from the rule by composing what exists and not from the kernels: de-interleave U and V, shift the containers to samples,
apply the planar restatement (resize_ref.resize_clip, which tests/test_resize_host.py holds against the C++ plan and the continuous
definition), shift back and re-interleave.  No row is copied: every output container has zero low bits, at equal sizes too.  And the port
of the rule that fits a wave's run of PAIRS of an interleaved UV row into its staging region (csrc/resize_region.h).  Checker side only."""
import resize_ref as R
import temporal_nr_surfaces_ref as TS

REGION_BYTES = R.REGION_BYTES
MAX_ZERO_TAPS = 7               # KR - K of the register forms (K <= 8 / 12 / 16) is largest at K = 1
PAIR_SLACK = 48                 # 15 bytes in front of an aligned-down span + 7 zero taps of one 4-byte pair each = 43, to the next 16


def register_taps(K):
    """taps a lane of the horizontal stage keeps in registers for a window of K (0: it walks the table and reads no zero tap)"""
    return 8 if K <= 8 else 12 if K <= 12 else 16 if K <= 16 else 0


def resize_surfaces(planes, dst_w, dst_h, bits, interleaved, msb, kernel="blackman", taps=None):
    """the destination's tight planes -- (Y, UV) interleaved, (Y, U, V) planar -- over the source's tight planes (containers as stored)"""
    out = R.resize_clip(TS.unpack(planes, bits, interleaved, msb), dst_w, dst_h, bits, kernel, taps)
    return TS.pack(out, bits, interleaved, msb)


def pair_columns_per_wave(S, D, es, kernel="blackman", taps=None):
    """(cpw, K, spans) of an interleaved UV row whose chroma axis is S -> D, from the rule's text: a wave's 64 lanes are up to 32 output
    columns times 2 components; it stages 2 * es * (start[last] + K - start[first]) bytes in a region of 2048 of which PAIR_SLACK are
    kept; the run is halved from 32 until every run of the row fits.  cpw 0, spans (): the run is refused on interleaved surfaces"""
    K, start = R.windows(S, D, kernel, taps)
    cpw = 32
    while cpw >= 1:
        spans = tuple(int(start[min(c0 + cpw, D) - 1] + K - start[c0]) * 2 * es for c0 in range(0, D, cpw))
        if all(s + PAIR_SLACK <= REGION_BYTES for s in spans):
            return cpw, K, spans
        cpw //= 2
    return 0, K, ()
