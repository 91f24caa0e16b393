// amt_gpu_tnr.hip -- C ABI part 6: temporal noise reduction, the reference's TemporalNRFilter (VideoFilter.hpp:27-212) over frames
// resident in HBM, byte for byte.  The window of output frame t is the clip's frames clamp(t + k, 0, clip_frames - 1),
// k = -d .. d, for a clip of any length.  Two entry points over one set of argument checks: amtgpu_temporal_nr takes planar LSB planes and
// nothing else; amtgpu_temporal_nr_surfaces takes every pair of descriptors in kind and runs the rule on samples (container >> shift).
#include "build_knobs.h"
#include "../../include/amt_gpu.h"

#include <string>

#include "api_common.hpp"
#include "plane_pair.hpp"

using namespace amt;

namespace {
const PlanePairRule& kPair = kTemporalNRPair;
const char* const kWho = kPair.who;

[[noreturn]] void refuse(const std::string& what) { throw std::runtime_error(std::string(kWho) + " " + what); }

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
    // the source/destination rule (plane_pair.hpp)
    const FrameBatch s = kPair.side("source", src, surface_batch(src, kWho), width, any_layout),
                     t = kPair.side("destination", dst, surface_batch(dst, kWho), width, any_layout);
    if (src->bits != dst->bits) refuse("source and destination differ in bits");
    kPair.in_kind(s, t);
    if (src_first < 0 || nsrc <= 0 || (long long)src_first + nsrc > clip_frames) refuse("the source batch does not lie inside the clip");
    if (out_first < 0 || (long long)out_first + nout > clip_frames) refuse("an output frame lies outside the clip");
    const long long last = (long long)clip_frames - 1, batch_end = (long long)src_first + nsrc;
    const long long wlo = std::max<long long>((long long)out_first - d, 0), whi = std::min<long long>((long long)out_first + nout - 1 + d, last);
    if (wlo < src_first || whi >= batch_end)
        refuse("window frame " + std::to_string(wlo < src_first ? wlo : whi) + " is outside the batch [" + std::to_string(src_first) + ", " + std::to_string(batch_end) + ")");

    const PlaneBytes sb = kPair.bytes(s, width, height), tb = kPair.bytes(t, width, height);
    kPair.disjoint(sb, nsrc, tb, nout);
    TemporalNRArgs a;
    pair_args(a, sb, tb);
    a.W = width; a.H = height;
    a.es = s.es;
    a.d = d; a.thresh = threshold << (src->bits - 8); a.interlaced = interlaced ? 1 : 0;
    a.first = out_first - src_first; a.lo = -src_first; a.hi = (int)(last - src_first);
    const bool planes = !s.interleaved && !s.shift;                                  // planar LSB: the planar kernel, as before
    a.vec = planes ? temporal_nr_vec16(sb.luma(), sb.chroma(), tb.luma(), tb.chroma())
                   : temporal_nr_surface_vec16(sb.luma(), sb.chroma(), tb.luma(), tb.chroma(), s.interleaved);
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
