// amt_gpu_edgelevel.hip -- C ABI part 9: the edge level behind the deband in the server's chain (KEdgeLevel(16, 10, 2), Misc.cs:1435; the
// GUI's "edge enhancement (for anime)" checkbox) over frames resident in HBM ("parity unpinned").  Stateless, as
// the temporal NR: there is no table, so no object.  Planar LSB planes only; decoder surfaces in kind are not built.
#include "build_knobs.h"
#include "../../include/amt_gpu.h"

#include <string>

#include "api_common.hpp"
#include "plane_pair.hpp"

using namespace amt;

namespace {
const auto& kPair = kEdgeLevelPair;                  // (plane_pair.hpp's rule in this entry point's words)
const char* const kWho = kPair.who;

[[noreturn]] void refuse(const std::string& what) { throw std::runtime_error(std::string(kWho) + " " + what); }

void edgelevel(AmtGpuContext* c, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int width, int height, int nframes, int strength, int threshold, int repair)
{
    if (strength < 0 || strength > 255) refuse("strength must be 0..255");
    if (threshold < 0 || threshold > 32767) refuse("threshold must be 0..32767");
    if (repair < 0 || repair > 4) refuse("repair must be 0..4");
    if (nframes < 0) refuse("negative frame count");
    if (nframes == 0) return;
    if (width <= 0 || height <= 0 || ((width | height) & 1)) refuse("width and height must be even and positive (4:2:0)");
    // the source/destination rule (plane_pair.hpp)
    const FrameBatch s = kPair.side("source", src, surface_batch(src, kWho), width, false),
                     t = kPair.side("destination", dst, surface_batch(dst, kWho), width, false);
    if (src->bits != dst->bits) refuse("source and destination differ in bits");
    kPair.in_kind(s, t);                                 // (planar LSB sides are in kind)
    const PlaneBytes sb = kPair.bytes(s, width, height), tb = kPair.bytes(t, width, height);
    kPair.disjoint(sb, nframes, tb, nframes);

    EdgeLevelArgs a;
    pair_args(a, sb, tb);
    a.W = width; a.H = height;
    a.es = s.es;
    a.vec = edgelevel_vec16(s.es, sb.luma(), sb.chroma(), tb.luma(), tb.chroma(), sb.row[0], sb.row[1]);
    a.strength = strength; a.thresh = threshold << (src->bits - 8); a.repair = repair;
    c->bind();
    const int sp_ = c->prof_begin("edgelevel_kernel");
    AMT_HIP(launch_edgelevel(c->stream, a, nframes));
    c->prof_end(sp_);
    AMT_HIP(hipStreamSynchronize(c->stream));            // as amtgpu_temporal_nr: dst is ready when the call returns
}
} // namespace

extern "C" {

int amtgpu_edgelevel(AmtGpuContext* c, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int width, int height, int nframes, int strength, int threshold,
                     int repair)
{
    if (!c) return 0;
    return guard(c, [&] { edgelevel(c, src, dst, width, height, nframes, strength, threshold, repair); });
}

} // extern "C"
