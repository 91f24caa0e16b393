"""Inputs for the two raw-buffer kernels (frame_stats_kernel, logofind_kernel) at the edges of their addressing, and deliberately
wrong restatements ("mutants") of both, in numpy only.

A batch is an ALLOCATION plus a view of it: frames of W x H samples at `base + n * frame_stride + y * pitch + x` (all in samples).
Everything of the allocation that is not a sample of a frame -- padding columns, gap rows between frames, what lies before the first
frame and after the last -- holds the container's top value (255 / 65535), so a kernel that reads it as a sample shows it in its sums.

The mutants model the allocation byte by byte, the way the kernels address it (tests/logofind_ref.py):
tests/test_plane_edge_inputs_host.py shows, without a GPU, that every input the GPU tests use tells the true result from each
mutant that applies to it.  The case lists at the end are shared by both test files.
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass, replace

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import frame_stats_oracle as FS
import logofind_ref as LF

COL_BYTES = 16                         # bytes of a row one lane of frame_stats_kernel owns
RUN = 32                               # frames a workgroup of frame_stats_kernel walks through
LF_LANE_COLS = 4                       # samples of a row one lane of logofind_kernel owns


# ---------------------------------------------------------------------------------------------------------------- form predictor
# RESTATES THE HOST RULES of launch_frame_stats (stats_kernels.hip) and logofind_grid (logofind_body.h): it has to move with them.
# The tests use it only to assert that their parameter lists reach every form; what a kernel computes is never taken from it.
def predicted_form(kernel, W, pitch, es):
    """'buf' / 'buf_ragged' / 'plain' for kernel == 'frame_stats', 'buf' / 'plain' for 'logofind'"""
    if kernel == "frame_stats":
        cols = -(-W * es // COL_BYTES)
        if cols * COL_BYTES > pitch * es:
            return "plain"
        return "buf_ragged" if (W * es) % COL_BYTES else "buf"
    if kernel == "logofind":
        return "buf" if -(-W // LF_LANE_COLS) * LF_LANE_COLS <= pitch else "plain"
    raise ValueError(kernel)


def tile_rows(form, es):
    """rows of a tile of frame_stats_kernel: 24 at 8 bits, 16 at 16 bits, 8 in the plain form (moves with stats_kernels.hip too)"""
    return 8 if form == "plain" else (24 if es == 1 else 16)


FRAME_STATS_FORMS = {(f, es) for f in ("buf", "buf_ragged", "plain") for es in (1, 2)}
LOGOFIND_FORMS = {(f, es) for f in ("buf", "plain") for es in (1, 2)}


# ---------------------------------------------------------------------------------------------------------------- allocations
@dataclass(frozen=True)
class Clip:
    buf: np.ndarray          # the flat allocation (uint8 or uint16)
    base: int                # first sample of frame 0, in samples from the start of the allocation
    frame_stride: int        # samples
    pitch: int               # samples
    W: int
    H: int
    N: int

    @property
    def es(self):
        return self.buf.dtype.itemsize

    @property
    def top(self):
        return 255 if self.es == 1 else 65535

    def view(self):
        """(base, frame stride, pitch, W, H, N), in samples"""
        return self.base, self.frame_stride, self.pitch, self.W, self.H, self.N

    def frames(self):
        """the samples: an (N, H, W) view of the allocation"""
        s = self.buf.strides[0]
        return np.lib.stride_tricks.as_strided(self.buf[self.base:], (self.N, self.H, self.W),
                                               (self.frame_stride * s, self.pitch * s, s), writeable=False)

    def sub(self, first, count=None):
        """frames [first, first + count) of the same allocation"""
        count = self.N - first if count is None else count
        assert 0 <= first and count >= 0 and first + count <= self.N
        return replace(self, base=self.base + first * self.frame_stride, N=count)

    def form(self, kernel="frame_stats"):
        return predicted_form(kernel, self.W, self.pitch, self.es)


def embed(samples, pitch, base=0, rows_before=0, rows_after=0, tail_rows=1):
    """samples (N, H, W) uint8 / uint16 -> Clip.  Frame n starts rows_before rows into a slot of rows_before + H + rows_after rows of
    `pitch` samples (a crop out of taller frames when either is > 0), the slots start `base` samples into the allocation, and
    tail_rows more rows follow the last frame; all of that poisoned with the top value."""
    samples = np.asarray(samples)
    N, H, W = samples.shape
    assert samples.dtype in (np.uint8, np.uint16) and pitch >= W and base >= 0
    stride = (rows_before + H + rows_after) * pitch
    first = base + rows_before * pitch
    size = first + (N - 1) * stride + H * pitch + tail_rows * pitch
    buf = np.full(size, np.iinfo(samples.dtype).max, samples.dtype)
    clip = Clip(buf, first, stride, pitch, W, H, N)
    f = np.lib.stride_tricks.as_strided(buf[first:], (N, H, W), tuple(k * buf.strides[0] for k in (stride, pitch, 1)))
    f[...] = samples
    return clip


def to_device(torch, dev, clip):
    """the batch as a device tensor view (N, H, pitch) of the same geometry over the whole allocation, poison included"""
    flat = torch.from_numpy(clip.buf.view(np.int16) if clip.es == 2 else clip.buf).to(dev)
    return torch.as_strided(flat, (clip.N, clip.H, clip.pitch), (clip.frame_stride, clip.pitch, 1), clip.base)


def orc_metrics(orc, clip, bits, prev=None):
    """orc_frame_metrics (the C restatement) on the same geometry; prev: a one-frame Clip of the same pitch, or None"""
    out = np.zeros((clip.N, 8), np.uint64)
    es = clip.es
    assert (bits <= 8) == (es == 1) and (prev is None or prev.pitch == clip.pitch)
    p = None if prev is None else prev.buf.ctypes.data + prev.base * es
    orc.lib.orc_frame_metrics(clip.buf.ctypes.data + clip.base * es, clip.frame_stride * es, clip.pitch, bits, clip.W, clip.H, clip.N,
                              p, out.ctypes.data)
    return out


def true_metrics(clip, prev=None):
    return FS.frame_metrics(clip.frames(), None if prev is None else prev.frames()[0])


def true_sums(clip):
    return LF.sums(clip.frames(), clip.W, clip.H)


# ---------------------------------------------------------------------------------------------------------------- mutants
@dataclass(frozen=True)
class Mutation:
    avg: str = "floor"               # 'ceil'; 16 bits, on packed dwords: 'no_shift_mask', 'no_carry_mask', 'no_masks'
    swap_parity: bool = False        # the weave takes its EVEN rows from the previous frame
    vrange: str = "inner"            # 'to_last': rows 1..H-1, 'from_first': rows 0..H-2
    rows_below: bool = False         # rows >= H of the last tile are read as stored
    pad_stored: bool = False         # padding bytes of a ragged last column are read as stored
    align: int = 1                   # every row's byte position rounded down to a multiple of this
    align_what: str = "offset"       # ... 'offset': inside the frame's buffer, 'address': inside the allocation
    before_is_n0: bool = False       # frame n0 - 1 of a run replaced by frame n0
    skip_odd_last: bool = False      # the last frame of an odd-length run (or launch) is skipped


FS_MUTANTS = {
    "avg_ceil": Mutation(avg="ceil"),
    "avg16_no_shift_mask": Mutation(avg="no_shift_mask"),
    "avg16_no_carry_mask": Mutation(avg="no_carry_mask"),
    "avg16_no_masks": Mutation(avg="no_masks"),
    "swap_parity": Mutation(swap_parity=True),
    "rows_1_to_last": Mutation(vrange="to_last"),
    "rows_0_to_inner": Mutation(vrange="from_first"),
    "rows_below_stored": Mutation(rows_below=True),
    "pad_stored": Mutation(pad_stored=True),
    "offset_align4": Mutation(align=4),
    "offset_align16": Mutation(align=16),
    "address_align4": Mutation(align=4, align_what="address"),
    "address_align16": Mutation(align=16, align_what="address"),
    "before_is_n0": Mutation(before_is_n0=True),
    "skip_odd_last": Mutation(skip_odd_last=True),
}
LF_MUTANTS = {k: FS_MUTANTS[k] for k in ("rows_1_to_last", "rows_0_to_inner", "offset_align4", "offset_align16", "address_align4",
                                         "address_align16", "skip_odd_last")}


def _row_positions(clip, mut, frame_byte):
    """byte position in the allocation of every row 0..H-1 of the frame that starts at frame_byte, as the mutation sees it"""
    off = np.arange(clip.H + 64, dtype=np.int64) * (clip.pitch * clip.es)
    if mut.align_what == "offset":
        return frame_byte + off // mut.align * mut.align
    return (frame_byte + off) // mut.align * mut.align


def _misaligned(clip, mut, prev=None):
    """does the mutation's rounding move any row of the batch (or of prev)?"""
    for c in (clip,) + ((prev,) if prev is not None else ()):
        for n in range(c.N):
            fb = (c.base + n * c.frame_stride) * c.es
            if not np.array_equal(_row_positions(c, mut, fb)[:c.H], fb + np.arange(c.H, dtype=np.int64) * (c.pitch * c.es)):
                return True
    return False


def fs_mutant_applies(name, clip, prev=None):
    """can the wrong kernel `name` differ from the right one on this geometry at all?  (Whether it DOES is what the host test shows.)"""
    m, form, es = FS_MUTANTS[name], clip.form(), clip.es
    if name == "avg16_no_shift_mask":
        return es == 2 and clip.W >= 2          # (the bit that mask stops comes out of a sample in the dword's high half)
    if name.startswith("avg16"):
        return es == 2
    if m.swap_parity:
        return clip.N > 1 or prev is not None        # (a frame woven with itself is itself either way)
    if m.rows_below:
        return clip.H % tile_rows(form, es) != 0
    if m.pad_stored:
        return form == "buf_ragged"
    if m.align > 1:
        return _misaligned(clip, m, prev)
    if m.before_is_n0:
        return clip.N > RUN
    if m.skip_odd_last:
        return clip.N % 2 == 1          # (runs are 32 frames: the last run is odd exactly when N is)
    return True


def lf_mutant_applies(name, clip):
    m = LF_MUTANTS[name]
    if m.align > 1:
        return _misaligned(clip, m)
    if m.skip_odd_last:
        return clip.N % 2 == 1
    return True


def _read(mem, pos, nbytes, es):
    """nbytes of the allocation from byte pos as samples; what lies outside the allocation reads as zero"""
    out = np.zeros(nbytes, np.uint8)
    a, b = max(0, pos), min(mem.size, pos + nbytes)
    if b > a:
        out[a - pos:b - pos] = mem[a:b]
    return out.view("<u2" if es == 2 else np.uint8).astype(np.int64)


def _fs_load(clip, mut, frame_byte):
    """the rows a (possibly wrong) frame_stats_kernel holds of one frame: (Hx + 2, Wx) int64, index r = row r - 1, where Hx is H rounded
    up to whole tiles and Wx the row rounded up to whole lane columns; zero wherever the right kernel reads zeros"""
    es, form = clip.es, clip.form()
    T = tile_rows(form, es)
    Hx = -(-clip.H // T) * T
    row_b = clip.W * es
    cols_b = -(-row_b // COL_BYTES) * COL_BYTES
    out = np.zeros((Hx + 2, cols_b // es), np.int64)
    mem = clip.buf.view(np.uint8)
    pos = _row_positions(clip, mut, frame_byte)
    take = cols_b if (mut.pad_stored and form == "buf_ragged") else row_b
    for y in range(Hx + 1 if mut.rows_below else clip.H):
        out[y + 1, :take // es] = _read(mem, int(pos[y]), take, es)
    return out


def _avg(a, c, how):
    if how == "floor":
        return (a + c) >> 1
    if how == "ceil":
        return (a + c + 1) >> 1
    # 16-bit samples two to a dword (even column: low half), Px<2>::avg with one or both of its masks left out
    pa, pc = a[..., 0::2] | (a[..., 1::2] << 16), c[..., 0::2] | (c[..., 1::2] << 16)
    sm = 0xFFFFFFFF if how in ("no_shift_mask", "no_masks") else 0x7FFF7FFF
    cm = 0xFFFFFFFF if how in ("no_carry_mask", "no_masks") else 0x00010001
    r = (((pa >> 1) & sm) + ((pc >> 1) & sm) + (pa & pc & cm)) & 0xFFFFFFFF
    out = np.empty_like(a)
    out[..., 0::2], out[..., 1::2] = r & 0xFFFF, r >> 16
    return out


def _fs_record(cur, prev, H, mut):
    Hx = cur.shape[0] - 2
    rec = np.zeros(8, np.uint64)
    d = np.abs(cur[1:Hx + 1] - prev[1:Hx + 1])
    rec[0], rec[1], rec[5] = d[0::2].sum(), d[1::2].sum(), cur[1:Hx + 1].sum()
    lo, hi = {"inner": (1, H - 2), "to_last": (1, H - 1), "from_first": (0, H - 2)}[mut.vrange]
    ys = np.arange(lo, hi + 1)
    weave = cur.copy()
    par = 0 if mut.swap_parity else 1
    weave[1 + par::2] = prev[1 + par::2]            # (index r = row r - 1)
    for X, kv, kc in ((cur, 2, 3), (weave, 6, 4)):
        a, b, c = X[ys], X[ys + 1], X[ys + 2]
        rec[kv] = np.abs(a - c).sum()
        rec[kc] = np.abs(b - _avg(a, c, mut.avg)).sum()
    return rec


def fs_model(clip, prev=None, mut=Mutation()):
    """(N, 8) uint64: the records frame_stats_kernel would write if it were wrong in the way `mut` says (Mutation(): the right ones)"""
    assert mut.avg in ("floor", "ceil") or clip.es == 2
    es = clip.es
    fb = lambda c, n: (c.base + n * c.frame_stride) * es
    out = np.zeros((clip.N, 8), np.uint64)
    for n0 in range(0, clip.N, RUN):
        n1 = min(clip.N, n0 + RUN)
        if n0 > 0:
            before = _fs_load(clip, mut, fb(clip, n0 if mut.before_is_n0 else n0 - 1))
        else:
            before = _fs_load(prev, mut, fb(prev, 0)) if prev is not None else _fs_load(clip, mut, fb(clip, 0))
        for n in range(n0, n1):
            cur = _fs_load(clip, mut, fb(clip, n))
            if not (mut.skip_odd_last and n == n1 - 1 and (n1 - n0) % 2 == 1):
                out[n] = _fs_record(cur, before, clip.H, mut)
            before = cur
    return out


def lf_model(clip, mut=Mutation()):
    """2 * W * H int64 (S1 then SM): the sums logofind_kernel would leave if it were wrong in the way `mut` says"""
    es, W, H = clip.es, clip.W, clip.H
    mem = clip.buf.view(np.uint8)
    n_end = clip.N - 1 if (mut.skip_odd_last and clip.N % 2 == 1) else clip.N
    Y = np.zeros((n_end, H + 2, W), np.int64)        # a ring row of zeros above and below
    for n in range(n_end):
        pos = _row_positions(clip, mut, (clip.base + n * clip.frame_stride) * es)
        for y in range(H):
            Y[n, y + 1] = _read(mem, int(pos[y]), W * es, es)
    S1 = Y[:, 1:-1].sum(0)
    SM = np.zeros_like(S1)
    lo, hi = {"inner": (1, H - 2), "to_last": (1, H - 1), "from_first": (0, H - 2)}[mut.vrange]
    ys = np.arange(lo, hi + 1)
    SM[lo:hi + 1, 1:-1] = (np.abs(Y[:, ys + 1, 2:] - Y[:, ys + 1, :-2]) + np.abs(Y[:, ys + 2, 1:-1] - Y[:, ys, 1:-1])).sum(0)
    return np.concatenate([S1.ravel(), SM.ravel()])


# ---------------------------------------------------------------------------------------------------------------- pictures
def dtype_of(bits):
    return np.uint8 if bits <= 8 else np.uint16


def random_frames(seed, N, H, W, bits):
    """uniform over the whole CONTAINER (0..255 / 0..65535), whatever depth is declared: the metrics are sums over stored values"""
    dt = dtype_of(bits)
    return np.random.RandomState(seed).randint(0, int(np.iinfo(dt).max) + 1, size=(N, H, W)).astype(dt)


def saturated_frames(N, H, W, bits, first=0):
    """frame n (numbered from `first`): rows of parity n % 2 at the top value, the others 0 -- every term of every row at its maximum"""
    dt = dtype_of(bits)
    Y = np.zeros((N, H, W), dt)
    for n in range(N):
        Y[n, (first + n) % 2::2] = np.iinfo(dt).max
    return Y


def vertical_pairs_8bit(Y):
    """(256, 256) bool: which (Y[y-1], Y[y+1]) pairs the frames hold"""
    have = np.zeros((256, 256), bool)
    have[Y[:, :-2].ravel(), Y[:, 2:].ravel()] = True
    return have


def full_range_frames_8bit(seed=0x5EED0081, N=5, H=240, W=352):
    """uniform 8-bit frames with the vertical (a, c) pairs that the draw missed planted: rows 4j and 4j + 2 of frame 0, one column each"""
    Y = random_frames(seed, N, H, W, 8)
    for rnd in range(4):                 # (a planted pair may overwrite the only copy of another: those go in the next round)
        for k, (a, c) in enumerate(np.argwhere(~vertical_pairs_8bit(Y))):
            j, x = divmod(k, W)
            Y[0, 4 * (j + 8 * rnd), x], Y[0, 4 * (j + 8 * rnd) + 2, x] = a, c
    return Y


EDGE_VALUES = (0, 1, 2, 0x7FFE, 0x7FFF, 0x8000, 0x8001, 0xFFFE, 0xFFFF)
EDGE_BLOCK = (3, 48, 64)              # frames, rows, columns
EDGE_AT = (1, 8)                      # row, column (even: the block keeps its column parities) of the block in its frames


def edge_block(seed=0x5EED00A7):
    """uniform draws from EDGE_VALUES (most draws of this size miss a triple or two: the seed is one that misses none, and the host
    test asserts it)"""
    return np.random.RandomState(seed).choice(np.array(EDGE_VALUES, np.uint16), size=EDGE_BLOCK)


def edge_triples(Y, parity):
    """the set of vertical triples (Y[y-1], Y[y], Y[y+1]) in the columns of one parity"""
    Y = np.asarray(Y)[:, :, parity::2].astype(np.int64)
    t = (Y[:, :-2] << 32) | (Y[:, 1:-1] << 16) | Y[:, 2:]
    return set(np.unique(t).tolist())


def all_edge_triples():
    return {(a << 32) | (b << 16) | c for a in EDGE_VALUES for b in EDGE_VALUES for c in EDGE_VALUES}


def full_range_frames_16bit(seed, N, H, W):
    """uniform over 0..65535 with the edge block in frames 0..2"""
    Y = random_frames(seed, N, H, W, 16)
    f, h, w = EDGE_BLOCK
    assert N >= f and H >= EDGE_AT[0] + h and W >= EDGE_AT[1] + w
    Y[:f, EDGE_AT[0]:EDGE_AT[0] + h, EDGE_AT[1]:EDGE_AT[1] + w] = edge_block()
    return Y


# ---------------------------------------------------------------------------------------------------------------- case lists
# Frame metrics.  A case is (bits, W, pitch, H, N, kwargs of embed); every clip is built with one frame more than N in front: the
# batch is frames 1..N, frame 0 the previous frame inside the same allocation.  16-bit cases declare 10 bits unless they say otherwise
# and hold full-range containers all the same.
FS_WIDTHS = {8: [(48, 48), (45, 48), (43, 48), (42, 48), (45, 45)],          # BUF whole rows; ragged with 1, 3, 2 bytes in the partial
             10: [(24, 24), (23, 24), (21, 24), (23, 23)]}                   # dword; plain


def _heights(bits, W, pitch):
    T = tile_rows(predicted_form("frame_stats", W, pitch, 1 if bits <= 8 else 2), 1 if bits <= 8 else 2)
    return [4, 5, T - 1, T, T + 1, T + 2, 2 * T + 1]


def _narrow(bits):
    es = 1 if bits <= 8 else 2
    out = []
    for W in (1, 2, 15, 16, 17):
        for pitch in sorted({W, -(-W * es // COL_BYTES) * COL_BYTES // es}):
            out.append((bits, W, pitch, 6, 3, {}))
    return out


GEOMETRY_CASES = ([(bits, W, pitch, H, 3, {}) for bits in (8, 10) for W, pitch in FS_WIDTHS[bits] for H in _heights(bits, W, pitch)]
                  + _narrow(8) + _narrow(10))

UNALIGNED_8 = [(352, 353), (352, 354), (352, 360), (350, 353)]
UNALIGNED_16 = [(176, 177), (176, 180), (173, 177)]
_CROP = dict(base=3, rows_before=2, rows_after=1)            # stride (H + 3) * pitch, first row 2, three columns in
ADDRESSING_CASES = (
    [(8, W, p, 50, 5, {}) for W, p in UNALIGNED_8] + [(10, W, p, 50, 5, {}) for W, p in UNALIGNED_16]
    # an aligned pitch, the base one sample in
    + [(8, 352, 352, 50, 5, dict(base=1)), (8, 350, 352, 50, 5, dict(base=1)), (10, 176, 176, 50, 5, dict(base=1)),
       (10, 173, 176, 50, 5, dict(base=1))]
    # crops out of taller, wider frames (350 in 351: the plain form)
    + [(8, 352, 360, 50, 5, _CROP), (8, 350, 353, 50, 5, _CROP), (8, 350, 351, 50, 5, _CROP), (10, 176, 180, 50, 5, _CROP),
       (10, 173, 177, 50, 5, _CROP), (10, 173, 174, 50, 5, _CROP)])
# the previous frame in an allocation of its own (another base, so another alignment)
SEPARATE_PREV_CASES = [(8, 352, 353, 50, 5, {}), (8, 350, 353, 50, 5, {}), (8, 350, 351, 50, 5, {}), (10, 176, 177, 50, 5, {}),
                       (10, 173, 177, 50, 5, {})]
BATCH_CASES = [(8, W, p, 26, N, {}) for W, p in ((48, 48), (45, 48)) for N in (1, 2, 31, 32, 33, 64, 65)]
DEALING_CASES = [(8, W, W, H, 2, {}) for W, H in ((16, 4000), (48, 1000), (2064, 50), (2032, 98))]
# (15: the deepest depth amtgpu_framestats_create takes; the containers hold 0 and 65535)
SATURATED_CASES = [(8, 48, 48, 25, 4, {}), (8, 45, 48, 25, 4, {}), (15, 24, 24, 17, 4, {}), (15, 23, 24, 17, 4, {})]
FULL_RANGE_8_CASES = [(8, 352, 352, 240, 5, {})]
FULL_RANGE_16_CASES = [(bits, W, 176, 50, 3, {}) for W in (176, 173) for bits in (10, 12, 15)]

FS_FAMILIES = dict(geometry=GEOMETRY_CASES, addressing=ADDRESSING_CASES, separate_prev=SEPARATE_PREV_CASES, batches=BATCH_CASES,
                   dealing=DEALING_CASES, full_range_8=FULL_RANGE_8_CASES, full_range_16=FULL_RANGE_16_CASES, saturated=SATURATED_CASES)
# the mutants every family has to tell apart in at least one of its inputs (and in EVERY input they apply to)
_ARITH = ["avg_ceil", "swap_parity", "rows_1_to_last", "rows_0_to_inner"]
_ARITH16 = ["avg16_no_shift_mask", "avg16_no_carry_mask", "avg16_no_masks"]
_ALIGN = ["offset_align4", "offset_align16", "address_align4", "address_align16"]
FS_FAMILY_MUTANTS = dict(geometry=_ARITH + _ARITH16 + ["rows_below_stored", "pad_stored"],
                         addressing=_ARITH + _ARITH16 + _ALIGN + ["rows_below_stored", "pad_stored"],
                         separate_prev=_ARITH + _ALIGN + ["pad_stored"],
                         batches=_ARITH + ["before_is_n0", "skip_odd_last", "rows_below_stored", "pad_stored"],
                         dealing=_ARITH + ["rows_below_stored"],
                         full_range_8=_ARITH,
                         full_range_16=_ARITH + _ARITH16 + ["rows_below_stored", "pad_stored"],
                         # (rows of one parity are equal, so avg is exact and both weaves are flat: the rounding and the parity
                         # mutants cannot show here; this family is about every term at its maximum)
                         saturated=["rows_1_to_last", "rows_0_to_inner"] + _ARITH16)


def forms_reached(kernel, cases):
    """{(form, sample size)} of a case list; a logo finder case carries its pitch fourth"""
    k = 2 if kernel == "frame_stats" else 3
    return {(predicted_form(kernel, c[1], c[k], 1 if c[0] <= 8 else 2), 1 if c[0] <= 8 else 2) for c in cases}


def case_id(case):
    bits, W, pitch, H, N, kw = case
    return f"{bits}b-{W}in{pitch}x{H}-n{N}" + "".join(f"-{k}{v}" for k, v in sorted(kw.items()))


def _seed(case):
    bits, W, pitch, H, N, kw = case
    return (bits * 1000003 + W * 7919 + pitch * 104729 + H * 31 + N + sum(kw.values())) & 0x7FFFFFFF


def fs_clip(case, family=None):
    """(clip of N + 1 frames, separate previous frame or None).  The batch is clip.sub(1); clip.sub(0, 1) the previous frame inside the
    allocation."""
    bits, W, pitch, H, N, kw = case
    if family == "saturated":
        Y = saturated_frames(N + 1, H, W, bits, first=-1)
    elif family == "full_range_8":
        Y = np.concatenate([random_frames(_seed(case), 1, H, W, 8), full_range_frames_8bit(N=N, H=H, W=W)])
    elif family == "full_range_16":
        Y = full_range_frames_16bit(_seed(case), N + 1, H, W)
        Y = np.concatenate([Y[-1:], Y[:-1]])              # the edge block in the batch's frames
    else:
        Y = random_frames(_seed(case), N + 1, H, W, bits)
    clip = embed(Y, pitch, **kw)
    prev = None
    if family == "separate_prev":
        prev = embed(random_frames(_seed(case) ^ 0x55AA, 1, H, W, bits), pitch, base=5)
    return clip, prev


# Logo finder: (bits, w, h, pitch, n, kwargs of embed)
LOGOFIND_CASES = ([(8, 61, 37, 65, 17, {}), (8, 250, 9, 253, 17, {}), (8, 600, 20, 601, 17, {}), (16, 61, 37, 65, 17, {}),
                   (16, 250, 9, 253, 17, {})]
                  # gapped, base offset: a crop
                  + [(8, 61, 37, 65, 17, _CROP), (16, 61, 37, 65, 17, _CROP), (8, 250, 9, 256, 17, _CROP)]
                  # the sample-by-sample form on the same crop (61 in 62: the last lane column would leave the row)
                  + [(8, 61, 37, 62, 17, _CROP), (16, 61, 37, 62, 17, _CROP)])
LOGOFIND_MUTANTS = list(LF_MUTANTS)


def lf_case_id(case):
    bits, w, h, pitch, n, kw = case
    return f"{bits}b-{w}x{h}in{pitch}-n{n}" + "".join(f"-{k}{v}" for k, v in sorted(kw.items()))


def lf_clip(case):
    bits, w, h, pitch, n, kw = case
    return embed(random_frames(_seed((bits, w, pitch, h, n, kw)), n, h, w, bits), pitch, **kw)
