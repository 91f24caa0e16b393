// amt_gpu_tnr.hip -- C ABI part 6: temporal noise reduction, the reference's TemporalNRFilter (VideoFilter.hpp:27-212) over frames
// resident in HBM, byte for byte.  The window of output frame t is the clip's frames clamp(t + k, 0, clip_frames - 1),
// k = -d .. d, for a clip of any length.  Two entry points over one set of argument checks: amtgpu_temporal_nr takes planar LSB planes and
// nothing else; amtgpu_temporal_nr_surfaces takes every pair of descriptors in kind and runs the rule on samples (container >> shift).
#include "build_knobs.h"
#include "../../include/amt_gpu.h"

#include <string>

#include "api_common.hpp"

using namespace amt;

namespace {
const char* const kWho = "[TemporalNR]";

[[noreturn]] void refuse(const std::string& what) { throw std::runtime_error(std::string(kWho) + " " + what); }

// surfaces with rows of at least width (chroma: width / 2 planar, 2 * (width / 2) interleaved) containers; any_layout: of every layout
// (amtgpu_temporal_nr_surfaces), else planar LSB planes only
FrameBatch tnr_surfaces(const AmtGpuSurfaces* s, const char* which, int width, bool any_layout)
{
    const FrameBatch b = surface_batch(s, kWho);
    if (!any_layout && (s->interleaved || s->msb_aligned))
        refuse(std::string(which) + ": planar, LSB-aligned planes only (interleaved and MSB-aligned surfaces are refused)");
    if (b.strideY < 0 || b.strideUV < 0) refuse(std::string(which) + ": negative frame stride");
    if (b.pitchY < width || b.pitchUV < (b.interleaved ? width : width / 2)) refuse(std::string(which) + ": pitch smaller than the row");
    return b;
}

// [first byte, one past the last byte) that n frames of a plane span
struct Span { uintptr_t lo, hi; };
Span plane_span(const void* p, long long stride, int pitch_bytes, int row_bytes, int rows, int n)
{
    const uintptr_t lo = (uintptr_t)p;
    return Span{lo, lo + (uintptr_t)(n - 1) * (uintptr_t)stride + (uintptr_t)(rows - 1) * (uintptr_t)pitch_bytes + (uintptr_t)row_bytes};
}

// both entry points: any_layout is amtgpu_temporal_nr_surfaces, which takes every pair in kind
void temporal_nr(AmtGpuContext* c, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height, int out_first, int nout,
                 int d, int threshold, int interlaced, const AmtGpuSurfaces* dst, bool any_layout)
{
    if (d < 0 || d > 63) refuse("temporal_distance must be 0..63");
    if (threshold < 0 || threshold > 32767) refuse("threshold must be 0..32767");
    if (nout < 0) refuse("negative output frame count");
    if (nout == 0) return;
    if (width <= 0 || height <= 0 || (width & 1) || (height & 1)) refuse("width and height must be even (4:2:0)");
    if (interlaced && height % 4) refuse("interlaced chroma needs a height that is a multiple of 4");
    const FrameBatch s = tnr_surfaces(src, "source", width, any_layout), t = tnr_surfaces(dst, "destination", width, any_layout);
    if (src->bits != dst->bits) refuse("source and destination differ in bits");
    if (s.interleaved != t.interleaved || s.shift != t.shift)
        refuse("source and destination are not in kind (equal bits, interleaved and MSB shift): the filter converts no layouts");
    if (src_first < 0 || nsrc <= 0 || (long long)src_first + nsrc > clip_frames) refuse("the source batch does not lie inside the clip");
    if (out_first < 0 || (long long)out_first + nout > clip_frames) refuse("an output frame lies outside the clip");
    const long long last = (long long)clip_frames - 1, batch_end = (long long)src_first + nsrc;
    const long long wlo = std::max<long long>((long long)out_first - d, 0), whi = std::min<long long>((long long)out_first + nout - 1 + d, last);
    if (wlo < src_first || whi >= batch_end)
        refuse("window frame " + std::to_string(wlo < src_first ? wlo : whi) + " is outside the batch [" + std::to_string(src_first) + ", " + std::to_string(batch_end) + ")");

    const int es = s.es, wUV = width >> 1, hUV = height >> 1;
    TemporalNRArgs a;
    a.srcY = (const uint8_t*)s.Y; a.srcU = (const uint8_t*)s.U; a.srcV = (const uint8_t*)s.V;
    a.dstY = (uint8_t*)t.Y; a.dstU = (uint8_t*)t.U; a.dstV = (uint8_t*)t.V;
    a.src_strideY = s.strideY; a.src_strideUV = s.strideUV; a.dst_strideY = t.strideY; a.dst_strideUV = t.strideUV;
    a.src_pitchY = s.pitchY * es; a.src_pitchUV = s.pitchUV * es; a.dst_pitchY = t.pitchY * es; a.dst_pitchUV = t.pitchUV * es;
    a.W = width; a.H = height;
    a.es = es;
    a.d = d; a.thresh = threshold << (src->bits - 8); a.interlaced = interlaced ? 1 : 0;
    a.first = out_first - src_first; a.lo = -src_first; a.hi = (int)(last - src_first);
    const int rowY = width * es, rowUV = (s.interleaved ? 2 * wUV : wUV) * es;
    const int nplanes = s.interleaved ? 2 : 3;                                       // Y, then U and V or the one UV plane
    // destination frames must not overlap each other, and no destination plane's span may touch a source plane's
    if (nout > 1 && (a.dst_strideY < (long long)(height - 1) * a.dst_pitchY + rowY || a.dst_strideUV < (long long)(hUV - 1) * a.dst_pitchUV + rowUV))
        refuse("destination frames overlap each other");
    const Span sspan[3] = {plane_span(a.srcY, a.src_strideY, a.src_pitchY, rowY, height, nsrc), plane_span(a.srcU, a.src_strideUV, a.src_pitchUV, rowUV, hUV, nsrc),
                           plane_span(a.srcV, a.src_strideUV, a.src_pitchUV, rowUV, hUV, nsrc)};
    const Span dspan[3] = {plane_span(a.dstY, a.dst_strideY, a.dst_pitchY, rowY, height, nout), plane_span(a.dstU, a.dst_strideUV, a.dst_pitchUV, rowUV, hUV, nout),
                           plane_span(a.dstV, a.dst_strideUV, a.dst_pitchUV, rowUV, hUV, nout)};
    for (int i = 0; i < nplanes; ++i)
        for (int j = 0; j < nplanes; ++j)
            if (const Span &x = sspan[i], &y = dspan[j]; x.lo < y.hi && y.lo < x.hi) refuse("the destination's byte range overlaps the source's (no in-place filtering)");
    const RowsAt srcY{lane_addr(a.srcY), 0, a.src_strideY, a.src_pitchY}, srcUV{lane_addr(a.srcU), lane_addr(a.srcV), a.src_strideUV, a.src_pitchUV};
    const RowsAt dstY{lane_addr(a.dstY), 0, a.dst_strideY, a.dst_pitchY}, dstUV{lane_addr(a.dstU), lane_addr(a.dstV), a.dst_strideUV, a.dst_pitchUV};
    const bool planes = !s.interleaved && !s.shift;                                  // planar LSB: the planar kernel, as before
    // (an interleaved batch has null V planes, which count as aligned: surface_batch drops whatever the descriptor holds there)
    a.vec = planes ? temporal_nr_vec16(srcY, srcUV, dstY, dstUV) : temporal_nr_surface_vec16(srcY, srcUV, dstY, dstUV, s.interleaved);
    c->bind();
    const int sp_ = c->prof_begin(planes ? "temporal_nr_kernel" : "temporal_nr_surfaces_kernel");
    AMT_HIP(planes ? launch_temporal_nr(c->stream, a, nout) : launch_temporal_nr_surfaces(c->stream, a, s.interleaved, s.shift, nout));
    c->prof_end(sp_);
    AMT_HIP(hipStreamSynchronize(c->stream));          // as amtgpu_kfm_render: dst is ready when the call returns
}
} // namespace

extern "C" {

int amtgpu_temporal_nr(AmtGpuContext* c, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height, int out_first, int nout,
                       int temporal_distance, int threshold, int interlaced, const AmtGpuSurfaces* dst)
{
    if (!c) return 0;
    return guard(c, [&] { temporal_nr(c, src, src_first, nsrc, clip_frames, width, height, out_first, nout, temporal_distance, threshold, interlaced, dst, false); });
}

int amtgpu_temporal_nr_surfaces(AmtGpuContext* c, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height, int out_first,
                                int nout, int temporal_distance, int threshold, int interlaced, const AmtGpuSurfaces* dst)
{
    if (!c) return 0;
    return guard(c, [&] { temporal_nr(c, src, src_first, nsrc, clip_frames, width, height, out_first, nout, temporal_distance, threshold, interlaced, dst, true); });
}

} // extern "C"
