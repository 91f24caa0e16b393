// lane_rule.h -- how many bytes one lane of a copy-shaped kernel may move: the largest of a few widths that divides EVERY address, frame
// stride, row pitch and row length the access is formed from.  It is the only thing between a caller's odd offset and a misaligned vector
// access, so it is written once, here, as pure functions of integers, and every launcher's selection is one named function below that the
// launcher calls with all of its operands.  No HIP in this file: tests/cpp/lane_rule_test.cpp compiles it with plain g++ and compares
// every selection with the expression the launchers used to write out by hand.
//
// All widths are powers of two, so "divides every operand" is "divides their OR"; a negative stride keeps its low bits as an unsigned.
#pragma once

#include <cstdint>

namespace amt {

inline uint64_t lane_addr(const void* p) { return (uint64_t)(uintptr_t)p; }

// Where the rows of one plane kind (luma, or both chroma planes) lie, in BYTES: the address of the first row of frame 0 in each plane
// (base2: the second chroma plane; 0 where there is none), bytes between frames, bytes between rows.
struct RowsAt {
    uint64_t base, base2;
    long long stride, pitch;
    uint64_t bits() const { return base | base2 | (uint64_t)stride | (uint64_t)pitch; }
};

inline bool lane_divides(uint64_t width, uint64_t bits) { return bits % width == 0; }
// the largest of wide > narrow that divides `bits`, else `least`
inline int lane_widest(uint64_t bits, int wide, int narrow, int least) { return lane_divides(wide, bits) ? wide : lane_divides(narrow, bits) ? narrow : least; }

// scan_keep_kernel: bytes per lane (16, 4 or one sample) of a luma or chroma row of `row` bytes.  A slot's rows start at multiples of the
// row length from the store's base, so base and row length cover the destination
inline int scan_keep_lane_bytes(int es, const RowsAt& src, uint64_t store, uint64_t store2, long long row)
{
    return lane_widest(src.bits() | store | store2 | (uint64_t)row, 16, 4, es);
}

// surfaces_extract_kernel, luma and planar chroma: bytes per lane (16, 4 or one sample); `row`: source bytes of a rectangle row
inline int extract_lane_bytes(int es, const RowsAt& src, const RowsAt& dst, long long row)
{
    return lane_widest(src.bits() | (uint64_t)row | dst.bits(), 16, 4, es);
}
// ... interleaved chroma: a lane stores half of what it loads to each plane -- 8-byte stores behind a 16-byte load, 2-byte stores behind a
// 4-byte one; pairwise: neither holds, the row goes pair by pair (bytes = 2 * es is then two loads of one sample)
struct SplitLanes { int bytes, pairwise; };
inline SplitLanes extract_split_lanes(int es, const RowsAt& src, const RowsAt& dst, long long row)
{
    const uint64_t s = src.bits() | (uint64_t)row, d = dst.bits();
    const bool quad = lane_divides(16, s) && lane_divides(8, d), one = lane_divides(4, s) && lane_divides(2, d);
    return SplitLanes{quad ? 16 : one ? 4 : 2 * es, one ? 0 : 1};
}

// delogo_surfaces_kernel: CONTAINERS per lane (4, 2 or 1) -- an access of n containers is naturally aligned.  src and dst are laid out
// alike; `row`: bytes of a rectangle row
inline int delogo_surface_lane_containers(int es, const RowsAt& src, const RowsAt& dst, long long row)
{
    return lane_widest(src.bits() | dst.bits() | (uint64_t)row, 4 * es, 2 * es, es) / es;
}

// delogo_kernel: may a lane take two samples at once -- every row start 2 * es aligned and the row an even number of samples.  `origin`:
// bytes from a row's start to the rectangle.  (Its four-sample form is a test of the row width alone, in the launcher.)
inline int delogo_pair_lanes(int es, const RowsAt& src, const RowsAt& dst, long long origin, long long row)
{
    return lane_divides(2 * (uint64_t)es, src.bits() | dst.bits() | (uint64_t)origin | (uint64_t)row) ? 1 : 0;
}

// ingest_rows_kernel: bytes per lane (16, 4 or 1) of chunks of `chunk` bytes
inline int ingest_lane_bytes(uint64_t src, uint64_t dst, long long src_stride, long long dst_stride, unsigned long long chunk)
{
    return lane_widest(src | dst | (uint64_t)src_stride | (uint64_t)dst_stride | (uint64_t)chunk, 16, 4, 1);
}

// the cadence renderer: 16-byte lanes where every row of every plane starts 16-byte aligned (the kernels finish a row's last bytes
// narrower, so the row length is no operand).  A null plane counts as aligned
inline int render_vec16(const RowsAt& srcY, const RowsAt& srcUV, const RowsAt& dstY, const RowsAt& dstUV)
{
    return lane_divides(16, srcY.bits() | srcUV.bits() | dstY.bits() | dstUV.bits()) ? 1 : 0;
}

// temporal_nr_surfaces_kernel: a lane takes 16 bytes of two luma rows and the chroma under them, where every luma row starts 16-byte
// aligned and so does what the lane takes of a chroma row: planar, an 8-byte run of the U and of the V row, so 8 bytes; interleaved, one
// 16-byte run of the UV row (base2 is 0: there is no V plane).  A row's last containers go two luma columns at a time, so the row length
// is no operand; otherwise the kernel goes container by container
inline int temporal_nr_surface_vec16(const RowsAt& srcY, const RowsAt& srcUV, const RowsAt& dstY, const RowsAt& dstUV, int interleaved)
{
    return lane_divides(16, srcY.bits() | dstY.bits()) && lane_divides(interleaved ? 16 : 8, srcUV.bits() | dstUV.bits()) ? 1 : 0;
}
// temporal_nr_kernel: planar planes
inline int temporal_nr_vec16(const RowsAt& srcY, const RowsAt& srcUV, const RowsAt& dstY, const RowsAt& dstUV)
{
    return temporal_nr_surface_vec16(srcY, srcUV, dstY, dstUV, 0);
}

// resize_h_kernel / resize_v_kernel: every plane goes on its own, so chroma rows are held to what luma rows are.  The horizontal stage
// stages a wave's source span with aligned 16-byte loads and the vertical stage gives a lane 16 bytes of an output row and of each
// intermediate row under it, where every row of the source, of the intermediate (`mid`, the object's own) and of the destination starts
// 16-byte aligned (a row's last containers go narrower, so the row length is no operand); otherwise both go container by container
inline int resize_vec16(const RowsAt& srcY, const RowsAt& srcUV, const RowsAt& midY, const RowsAt& midUV, const RowsAt& dstY, const RowsAt& dstUV)
{
    return lane_divides(16, srcY.bits() | srcUV.bits() | midY.bits() | midUV.bits() | dstY.bits() | dstUV.bits()) ? 1 : 0;
}

// resize_surface_h_kernel / resize_surface_v_kernel: the same rule.  An interleaved UV plane is one plane whose rows are staged and
// walked 16 bytes at a time like any other (base2 is 0: there is no V plane, and a null plane counts as aligned)
inline int resize_surface_vec16(const RowsAt& srcY, const RowsAt& srcUV, const RowsAt& midY, const RowsAt& midUV, const RowsAt& dstY, const RowsAt& dstUV)
{
    return resize_vec16(srcY, srcUV, midY, midUV, dstY, dstUV);
}

// deband_kernel: every plane goes on its own.  A workgroup stages its tile's rows with aligned 16-byte loads and a lane stores 16 bytes
// of an output row, where every row of every plane of the source and of the destination starts 16-byte aligned (a row's last containers
// go narrower, so the row length is no operand); otherwise both go container by container
inline int deband_vec16(const RowsAt& srcY, const RowsAt& srcUV, const RowsAt& dstY, const RowsAt& dstUV)
{
    return lane_divides(16, srcY.bits() | srcUV.bits() | dstY.bits() | dstUV.bits()) ? 1 : 0;
}

// edgelevel_kernel: a lane loads 16 bytes of each luma row of its window and stores 16 bytes of an output row, and a chroma row is
// copied 16 bytes per lane, where every row of every plane of the source and of the destination starts 16-byte aligned.  `rowY` /
// `rowUV`: the BYTES of a luma / chroma row, the same on both sides.  A row's last containers go container by container, but the two
// containers beside a wave's span are loaded as one pair (lanes 0 and 63), which lies inside the row, and is aligned, only where the
// luma row is a whole number of pairs; a chroma row need only be whole containers.  Otherwise everything goes container by container
inline int edgelevel_vec16(int es, const RowsAt& srcY, const RowsAt& srcUV, const RowsAt& dstY, const RowsAt& dstUV, long long rowY, long long rowUV)
{
    return lane_divides(16, srcY.bits() | srcUV.bits() | dstY.bits() | dstUV.bits()) && lane_divides(2 * (uint64_t)es, (uint64_t)rowY) &&
                   lane_divides((uint64_t)es, (uint64_t)rowUV)
               ? 1
               : 0;
}

} // namespace amt
