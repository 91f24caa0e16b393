"""Inputs for the two copy kernels every frame enters through (ingest_kernels.hip): weave_fields_kernel (amtgpu_weave_fields_batch[_msb])
and ingest_rows_kernel (amtgpu_frames_upload_strided / _gather, amtgpu_download_strided), in numpy only.

Both kernels come in forms that the library picks at run time from the geometry it is handed -- 16-byte vectors or single elements
for the weave, 16-, 4- or 1-byte lanes for the row copies -- so a case here is a GEOMETRY: flat byte buffers with given pitches, frame
gaps and base offsets, all counted from the start of a 16-byte-aligned allocation.  Whatever is not a sample (guards in front and
behind, pitch padding, gaps) holds SENTINEL, and the tests compare whole buffers.

tests/test_copy_cases_host.py shows without a GPU that every case reaches the form, tail and number of rounds it is listed for;
tests/test_gpu_weave_forms.py and tests/test_gpu_row_copies.py run them.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from math import gcd

import numpy as np

GUARD = 64                             # bytes in front of and behind every weave plane (a multiple of 16)
SENTINEL = 0xA5
P, N = 5, 6                            # pictures, output frames
# every picture as top and as bottom; top != bottom in both orders (0,1 / 1,0); repeats (2 twice in each, once with itself)
TOP = (0, 1, 2, 3, 4, 2)
BOTTOM = (1, 0, 3, 4, 2, 2)
PLANES = ("srcY", "srcU", "srcV", "dstY", "dstU", "dstV")


def ceil_div(a, b):
    return -(-a // b)


def first_difference(got, want):
    """'' when the byte buffers are equal, else where they first differ (for assertion messages)"""
    got, want = np.asarray(got).view(np.uint8).ravel(), np.asarray(want).view(np.uint8).ravel()
    if got.size != want.size:
        return f"{got.size} bytes, expected {want.size}"
    bad = np.flatnonzero(got != want)
    if not bad.size:
        return ""
    return f"{bad.size} bytes differ, the first at {bad[0]}: {got[bad[0]]:#x}, expected {want[bad[0]]:#x}"


# ---------------------------------------------------------------------------------------------------------------- the weave
@dataclass(frozen=True)
class WeaveCase:
    name: str
    W: int
    H: int
    bits: int
    src_pitch: tuple                   # (Y, UV) in containers
    dst_pitch: tuple
    nv12: bool = False
    msb: bool = False
    off: dict = field(default_factory=dict)      # plane -> bytes its base is moved into the allocation
    gap: dict = field(default_factory=dict)      # "srcY" / "srcUV" / "dstY" / "dstUV" -> bytes left behind every frame of the plane(s)
    # what the case is listed for: the form the host selects, row bytes % 16 (luma, chroma) and rounds a wave makes per row (luma, chroma)
    form: str = "vec"
    tail: tuple = (0, 0)
    rounds: tuple = (1, 1)

    @property
    def es(self):
        return 1 if self.bits <= 8 else 2

    @property
    def shift(self):
        return 16 - self.bits if self.msb else 0

    @property
    def dtype(self):
        return np.dtype(np.uint8 if self.es == 1 else "<u2")


@dataclass(frozen=True)
class Plane:
    """one plane of a case inside its flat buffer, in bytes"""
    base: int
    stride: int
    pitch: int
    frames: int
    rows: int
    row: int
    size: int


def plane(case, which):
    src, luma = which.startswith("src"), which.endswith("Y")
    es = case.es
    rows = case.H if luma else case.H // 2
    pitch = (case.src_pitch if src else case.dst_pitch)[0 if luma else 1] * es
    row = (case.W if luma or (src and case.nv12) else case.W // 2) * es
    assert pitch >= row
    frames = P if src else N
    stride = rows * pitch + case.gap.get(which[:3] + ("Y" if luma else "UV"), 0)
    base = GUARD + case.off.get(which, 0)
    return Plane(base, stride, pitch, frames, rows, row, ceil_div(base + frames * stride + GUARD, 16) * 16)


def planes_of(case):
    return [w for w in PLANES if not (case.nv12 and w == "srcV")]


def samples(case, which, buf):
    """the (frames, rows, containers per row) view of a plane's flat uint8 buffer"""
    pl = plane(case, which)
    flat = buf[pl.base:].view(case.dtype)
    es = case.es
    return np.lib.stride_tricks.as_strided(flat, (pl.frames, pl.rows, pl.row // es), (pl.stride, pl.pitch, es))


def blank(case, which):
    return np.full(plane(case, which).size, SENTINEL, np.uint8)


def weave_source(case):
    """{plane: flat uint8 buffer} of P pictures: full-range random containers (the plain form copies them, the MSB form shifts them)"""
    rng = np.random.default_rng(case.W * 1009 + case.H * 31 + case.bits)          # (cases of one shape hold the same pictures)
    out = {}
    for w in planes_of(case)[:-3]:
        out[w] = blank(case, w)
        v = samples(case, w, out[w])
        v[...] = rng.integers(0, 256 ** case.es, v.shape).astype(case.dtype)
    return out


def weave(Y, U, V, top, bottom, nv12, shift=0):
    """The definition.  Y (P, H, W), U / V (P, H/2, W/2) containers, or U = the interleaved plane (P, H/2, W) and V None for NV12;
    frame i takes its even rows from picture top[i] and its odd rows from picture bottom[i], per plane; MSB containers are read as
    container >> shift."""
    top, bottom = np.asarray(top), np.asarray(bottom)
    if nv12:
        U, V = U[:, :, 0::2], U[:, :, 1::2]
    out = []
    for pl in (Y, U, V):
        f = pl[top].copy()
        f[:, 1::2] = pl[bottom][:, 1::2]
        out.append(f >> shift)
    return out


def weave_expected(case, src, top, bottom, nframes):
    """{plane: flat uint8 buffer} of the destination after weaving nframes frames (top / bottom None: frame i from picture i)"""
    ident = np.arange(nframes)
    top = ident if top is None else np.asarray(top)[:nframes]
    bottom = ident if bottom is None else np.asarray(bottom)[:nframes]
    Y, U = samples(case, "srcY", src["srcY"]), samples(case, "srcU", src["srcU"])
    V = None if case.nv12 else samples(case, "srcV", src["srcV"])
    out = {}
    for w, f in zip(PLANES[3:], weave(Y, U, V, top, bottom, case.nv12, case.shift)):
        out[w] = blank(case, w)
        samples(case, w, out[w])[:nframes] = f
    return out


# RESTATES THE HOST RULE of weave_fields() (amt_gpu_ingest.hip) and the loop steps of weave_fields_kernel: it has to move with them.
# The tests use it only to assert that the table reaches every form; what the kernel writes is never taken from it.
def weave_form(case):
    al16 = lambda pl: pl.base % 16 == 0 and pl.stride % 16 == 0 and pl.pitch % 16 == 0
    checked = ["srcY", "dstY", "dstU", "dstV"] + ([] if case.nv12 else ["srcU", "srcV"])
    return "vec" if all(al16(plane(case, w)) for w in checked) else "elem"


def weave_tails(case):
    return (case.W * case.es % 16, case.W // 2 * case.es % 16)


def weave_rounds(case):
    """rounds a wave makes per luma row and per chroma row: 1024 bytes a round on the vector path, 64 on the element path (128 in the
    shifting kernel, which moves containers); the NV12 split moves 64 samples a round whatever the form"""
    step = 1024 if weave_form(case) == "vec" else (128 if case.shift else 64)
    chroma = ceil_div(case.W // 2, 64) if case.nv12 else ceil_div(case.W // 2 * case.es, step)
    return (ceil_div(case.W * case.es, step), chroma)


_C1 = dict(W=96, H=12, bits=8, src_pitch=(96, 48), dst_pitch=(96, 48))       # H = 12: both plane boundaries inside an 8-row workgroup
_C10 = dict(W=192, H=12, bits=8, src_pitch=(192, 192), dst_pitch=(192, 96), nv12=True, rounds=(1, 2))
_C12 = dict(W=132, H=12, bits=10, src_pitch=(136, 136), dst_pitch=(136, 72), nv12=True, tail=(8, 4), rounds=(1, 2))
WEAVE_CASES = [
    WeaveCase("01-vec-whole", **_C1),
    WeaveCase("02-vec-tails", 90, 12, 8, (96, 48), (112, 64), tail=(10, 13)),
    WeaveCase("03-vec-three-rounds", 2090, 4, 8, (2096, 1056), (2096, 1056), tail=(10, 5), rounds=(3, 2)),
    WeaveCase("04-vec-16bit", 1050, 4, 16, (1056, 528), (1056, 528), tail=(4, 10), rounds=(3, 2)),
    WeaveCase("04-vec-12bit-msb", 1050, 4, 12, (1056, 528), (1056, 528), msb=True, tail=(4, 10), rounds=(3, 2)),
    WeaveCase("05-elem-by-pitch", 90, 12, 8, (91, 46), (91, 46), form="elem", tail=(10, 13), rounds=(2, 1)),
    WeaveCase("06-elem-by-dstY-base", **_C1, off={"dstY": 4}, form="elem", rounds=(2, 1)),
    WeaveCase("07-elem-by-srcV-base", **_C1, off={"srcV": 2}, form="elem", rounds=(2, 1)),
    WeaveCase("08-elem-by-8-byte-gap", **_C1, gap={"srcY": 8}, form="elem", rounds=(2, 1)),
    WeaveCase("09-vec-16-byte-gap", **_C1, gap={"srcY": 16}),
    WeaveCase("10-nv12-two-split-rounds", **_C10),
    WeaveCase("11-nv12-uv-base-moved", **_C10, off={"srcU": 2}),
    WeaveCase("12-nv12-10bit", **_C12),
    WeaveCase("12-nv12-10bit-msb", **_C12, msb=True),
    WeaveCase("13-elem-10bit-msb", 70, 12, 10, (71, 36), (80, 40), msb=True, form="elem", tail=(12, 6), rounds=(2, 1)),
    WeaveCase("14-16bit", 96, 12, 16, (96, 48), (96, 48)),
    WeaveCase("14-16bit-msb", 96, 12, 16, (96, 48), (96, 48), msb=True),
]


# ---------------------------------------------------------------------------------------------------------------- row copies
GRID_PASS = 2048 * 256                 # lanes of one pass of ingest_rows_kernel's grid


# RESTATES launch_ingest_rows (ingest_kernels.hip; ingest_lane_bytes, lane_rule.h); byte offsets are relative to 16-byte-aligned allocations.  Used only to assert
# that the tables reach every lane width.
def row_lanes(src_off, src_stride, dst_off, dst_stride, chunk):
    a = src_off | src_stride | dst_off | dst_stride | chunk
    return 16 if a % 16 == 0 else 4 if a % 4 == 0 else 1


@dataclass(frozen=True)
class RowCase:
    chunk: int
    pitch: int                         # of the device image
    off: int                           # bytes the device image's base is moved
    nchunks: int
    lanes: int                         # bytes a lane moves: what the case is listed for

    @property
    def id(self):
        return f"{self.chunk}in{self.pitch}+{self.off}x{self.nchunks}"


# through the staging ring the source is a slot (256-byte aligned) with the chunks back to back: the device side decides
STRIDED_UPLOADS = [RowCase(304, 320, 0, 37, 16), RowCase(304, 320, 4, 37, 4), RowCase(304, 320, 2, 37, 1), RowCase(304, 324, 0, 37, 4),
                   RowCase(301, 320, 0, 37, 1), RowCase(1, 16, 0, 37, 1), RowCase(304, 320, 0, 1, 16),
                   RowCase(701, 704, 0, 3000, 1)]                                  # 2.1 M lanes: more than one pass of the grid
# the device side of the download: the landing buffer is page-aligned with the chunks back to back
DOWNLOADS = STRIDED_UPLOADS[:3]
# a registered pool is read where it lies: (offset into the pool, source stride) -> lanes, the device image permitting 16 bytes
POOL_CASE = STRIDED_UPLOADS[0]
POOL_SOURCES = {(0, 2048): 16, (4, 2048): 4, (1, 2048): 1, (0, 2049): 1, (4, 2049): 1, (1, 2049): 1}
# across two slots of the ring (32 MiB each): 6 + 2 chunks of the strided call; 10 + 2 of the gather, the cut inside the third source
SLOT_BYTES = 32 << 20
TWO_SLOT_STRIDED = RowCase((5 << 20) + 4, (5 << 20) + 16, 0, 8, 4)
TWO_SLOT_GATHER = RowCase((3 << 20) + 4, (3 << 20) + 16, 0, 12, 4)
GATHER_SOURCES, GATHER_CHUNKS_PER_SOURCE = 3, 4
# separately allocated sources at odd addresses: staging packs them, so the lanes are the chunk's
SMALL_GATHERS = [RowCase(304, 320, 0, 35, 16), RowCase(301, 320, 0, 35, 1)]


@dataclass(frozen=True)
class Image:
    """rows of `chunk` bytes, `pitch` apart, inside a flat buffer with whole guard rows (a multiple of 16 bytes) on both sides"""
    base: int
    pitch: int
    chunk: int
    nchunks: int
    size: int

    def rows(self, buf):
        return np.lib.stride_tricks.as_strided(buf[self.base:], (self.nchunks, self.chunk), (self.pitch, 1))

    def blank(self):
        return np.full(self.size, SENTINEL, np.uint8)

    def holding(self, rows):
        buf = self.blank()
        self.rows(buf)[...] = rows
        return buf


def image(chunk, pitch, off, nchunks):
    assert pitch >= chunk
    guard = pitch * (16 // gcd(pitch, 16))
    return Image(guard + off, pitch, chunk, nchunks, ceil_div(guard + off + nchunks * pitch + guard, 16) * 16)


def random_rows(seed, nchunks, chunk):
    return np.random.default_rng(seed).integers(0, 256, (nchunks, chunk), dtype=np.uint8)
