// plane_pair.hpp -- the source/destination rule of the resident post-process chain (render, resize, temporal NR, deband, edge level; include/amt_gpu.h,
// "source and destination"): the only code between a caller's two descriptors and a kernel that writes HBM through them, so it is written
// once, here.  An entry point calls, in this order and with its own checks in between: side() on the source and on the destination,
// in_kind(), bytes() for either side, disjoint().  Every refusal is a std::runtime_error in the entry point's own words (PlanePairRule).
// No HIP in this file: tests/cpp/plane_pair_test.cpp compiles it with plain g++ and checks disjoint() against a map of bytes.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../include/amt_gpu.h"
#include "frame_batch.h"
#include "lane_rule.h"

namespace amt {

// [first byte, one past the last byte) that n frames of a plane span
struct Span { uintptr_t lo, hi; };
inline Span plane_span(const void* p, long long stride, long long pitch_bytes, int row_bytes, int rows, int n)
{
    const uintptr_t lo = (uintptr_t)p;
    return Span{lo, lo + (uintptr_t)(n - 1) * (uintptr_t)stride + (uintptr_t)(rows - 1) * (uintptr_t)pitch_bytes + (uintptr_t)row_bytes};
}

// One side's planes in BYTES, formed once (PlanePairRule::bytes): the planes there are -- Y, U, V, or Y and the one UV plane, whose rows
// are as many containers as luma rows; p[2] is null then, whatever the descriptor held -- and per plane kind [luma, chroma] the bytes
// between frames, between rows and of a row's samples, and the rows.  Pitches fit an int: bytes() refuses the others.
struct PlaneBytes {
    const void* p[3];
    int nplanes;
    long long stride[2];
    int pitch[2], row[2], rows[2];
    // what the lane rules take (lane_rule.h); a null plane counts as aligned
    RowsAt luma() const { return RowsAt{lane_addr(p[0]), 0, stride[0], pitch[0]}; }
    RowsAt chroma() const { return RowsAt{lane_addr(p[1]), lane_addr(p[2]), stride[1], pitch[1]}; }
    Span span(int plane, int n) const { const int k = plane ? 1 : 0; return plane_span(p[plane], stride[k], pitch[k], row[k], rows[k], n); }
};

// the pointers, strides and pitches of kernel arguments that name them srcY .. dst_pitchUV (TemporalNRArgs, RenderArgs)
template <typename Args> inline void pair_args(Args& a, const PlaneBytes& s, const PlaneBytes& t)
{
    a.srcY = (const uint8_t*)s.p[0]; a.srcU = (const uint8_t*)s.p[1]; a.srcV = (const uint8_t*)s.p[2];
    a.dstY = (uint8_t*)t.p[0]; a.dstU = (uint8_t*)t.p[1]; a.dstV = (uint8_t*)t.p[2];
    a.src_strideY = s.stride[0]; a.src_strideUV = s.stride[1]; a.dst_strideY = t.stride[0]; a.dst_strideUV = t.stride[1];
    a.src_pitchY = s.pitch[0]; a.src_pitchUV = s.pitch[1]; a.dst_pitchY = t.pitch[0]; a.dst_pitchUV = t.pitch[1];
}

// does a stride let the second of ndst destination frames begin inside the first, in luma or chroma
inline bool frames_overlap(const PlaneBytes& t, int ndst)
{
    for (int k = 0; k < 2; ++k)
        if (ndst > 1 && t.stride[k] < (long long)(t.rows[k] - 1) * t.pitch[k] + t.row[k]) return true;
    return false;
}
// does the span of a plane of t over ndst frames touch the span of a plane of s over nsrc frames
inline bool planes_touch(const PlaneBytes& s, int nsrc, const PlaneBytes& t, int ndst)
{
    for (int i = 0; i < s.nplanes; ++i)
        for (int j = 0; j < t.nplanes; ++j)
            if (const Span x = s.span(i, nsrc), y = t.span(j, ndst); x.lo < y.hi && y.lo < x.hi) return true;
    return false;
}

// The rule in one entry point's words: who refuses ("[Resize]"), what converts no layouts ("resizer"), the parenthesis behind an
// overlap ("(no in-place resize)"), and the object that was created for one depth ("resizer"; null: the entry point has none).
struct PlanePairRule {
    const char *who, *converter, *in_place, *object;

    [[noreturn]] void refuse(const std::string& what) const { throw std::runtime_error(std::string(who) + " " + what); }

    // One side (`which`: "source" / "destination"): s is the descriptor and b what surface_batch made of it, which is returned.  Rows of
    // at least width containers (chroma: width / 2 planar, width interleaved); any_layout: every layout is taken, else planar LSB
    // planes only; object_bits: the depth the object was created for
    FrameBatch side(const char* which, const AmtGpuSurfaces* s, const FrameBatch& b, int width, bool any_layout, int object_bits = 0) const
    {
        const std::string side = std::string(which) + ": ";
        if (!any_layout && (s->interleaved || s->msb_aligned)) refuse(side + "planar, LSB-aligned planes only (interleaved and MSB-aligned surfaces are refused)");
        if (object && s->bits != object_bits)
            refuse(side + std::to_string(s->bits) + " bits, the " + object + " was created for " + std::to_string(object_bits));
        if (b.strideY < 0 || b.strideUV < 0) refuse(side + "negative frame stride");
        if (b.pitchY < width || b.pitchUV < (b.interleaved ? width : width / 2)) refuse(side + "pitch smaller than the row");
        return b;
    }

    void in_kind(const FrameBatch& s, const FrameBatch& t) const
    {
        if (s.interleaved != t.interleaved || s.shift != t.shift)
            refuse(std::string("source and destination are not in kind (equal bits, interleaved and MSB shift): the ") + converter + " converts no layouts");
    }

    // a side of width x height luma containers in bytes.  The pitch is formed in 64 bits: the kernels take it as an int
    PlaneBytes bytes(const FrameBatch& b, int width, int height) const
    {
        const long long pitchY = (long long)b.pitchY * b.es, pitchUV = (long long)b.pitchUV * b.es;
        if (pitchY > INT32_MAX || pitchUV > INT32_MAX) refuse("pitch above 2 GiB");
        return PlaneBytes{{b.Y, b.U, b.interleaved ? nullptr : b.V}, b.interleaved ? 2 : 3, {b.strideY, b.strideUV}, {(int)pitchY, (int)pitchUV},
                          {width * b.es, (b.interleaved ? width : width / 2) * b.es}, {height, height / 2}};
    }

    // nsrc frames of s are read and ndst frames of t written, each side of its own size
    void disjoint(const PlaneBytes& s, int nsrc, const PlaneBytes& t, int ndst) const
    {
        if (frames_overlap(t, ndst)) refuse("destination frames overlap each other");
        if (planes_touch(s, nsrc, t, ndst)) refuse(std::string("the destination's byte range overlaps the source's ") + in_place);
    }
};

// the chain's entry points (each has a planar-LSB-only form and one that takes every pair in kind; all ask in_kind)
inline constexpr PlanePairRule kRenderPair{"[KFMRender]", "renderer", "(no in-place rendering)", nullptr};
inline constexpr PlanePairRule kResizePair{"[Resize]", "resizer", "(no in-place resize)", "resizer"};
inline constexpr PlanePairRule kTemporalNRPair{"[TemporalNR]", "filter", "(no in-place filtering)", nullptr};
inline constexpr PlanePairRule kDebandPair{"[Deband]", "filter", "(no in-place filtering: the filter reads neighbours)", "debander"};
// (planar LSB only so far)
inline constexpr PlanePairRule kEdgeLevelPair{"[EdgeLevel]", "filter", "(no in-place filtering: the filter reads neighbours)", nullptr};

} // namespace amt
