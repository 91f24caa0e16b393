// amt_gpu_render.hip -- C ABI part 5: the pictures that go with the cadence decisions (self-specified, "parity unpinned"; DESIGN.md
// section 6d): the render plan from cadence / phase, and the weave / bob renderer over source frames resident in HBM -- planes or
// decoder surfaces (NV12, P010 / P012, planar MSB), source and destination in kind.
#include "build_knobs.h"
#include "../../include/amt_gpu.h"

#include <string>
#include <vector>

#include "api_common.hpp"
#include "plane_pair.hpp"
#include "stats_decisions.hpp"

using namespace amt;

static_assert(sizeof(AmtGpuRenderFrame) == sizeof(RenderFrame) && sizeof(RenderFrame) == 16, "the plan entry of the ABI is the planner's");
static_assert(AMTGPU_RENDER_WEAVE == kRenderWeave && AMTGPU_RENDER_BOB_TOP == kRenderBobTop && AMTGPU_RENDER_BOB_BOTTOM == kRenderBobBottom,
              "the kinds of the ABI are the planner's");

namespace {
const PlanePairRule& kPair = kRenderPair;
const char* const kWho = kPair.who;

[[noreturn]] void refuse(const std::string& what) { throw std::runtime_error(std::string(kWho) + " " + what); }

// all entry points: deint LINE is amtgpu_kfm_render, ADAPTIVE the edge-directed, motion-adaptive rule -- on planes, and with
// adaptive_surfaces (amtgpu_kfm_render_deint_surfaces) on every pair in kind
void render(AmtGpuContext* c, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height, const AmtGpuRenderFrame* plan, int nout,
            int deint, int thresh, const AmtGpuSurfaces* dst, bool adaptive_surfaces = false)
{
    if (deint != AMTGPU_DEINT_LINE && deint != AMTGPU_DEINT_ADAPTIVE) refuse("deint " + std::to_string(deint) + " is neither AMTGPU_DEINT_LINE nor AMTGPU_DEINT_ADAPTIVE");
    const bool adaptive = deint == AMTGPU_DEINT_ADAPTIVE;
    if (adaptive && thresh != -1) refuse("the adaptive rule has no threshold: thresh must be -1");
    if (nout < 0) refuse("negative output frame count");
    if (nout == 0) return;
    if (!plan) refuse("null plan");
    if (width <= 0 || height < 4 || (width & 1) || (height & 1)) refuse("width and height must be even and height at least 4 (4:2:0 field pairs)");
    // the source/destination rule (plane_pair.hpp), surfaces in any layout
    const FrameBatch s = kPair.side("source", src, surface_batch(src, kWho), width, true), d = kPair.side("destination", dst, surface_batch(dst, kWho), width, true);
    if (src->bits != dst->bits) refuse("source and destination differ in bits");
    kPair.in_kind(s, d);
    if (adaptive && !adaptive_surfaces && (s.interleaved || s.shift)) refuse("the adaptive rule takes planes only (planar, LSB-aligned): interleaved and MSB-aligned surfaces are refused");
    if (src_first < 0 || nsrc <= 0 || (long long)src_first + nsrc > clip_frames) refuse("the source batch does not lie inside the clip");
    const int maxv = s.shift ? (1 << src->bits) - 1 : s.es == 1 ? 255 : 65535;      // of a sample: MSB-aligned ones are compared shifted

    std::vector<RenderEntry> entries((size_t)(adaptive ? 0 : nout));
    std::vector<RenderAdaptiveEntry> aentries((size_t)(adaptive ? nout : 0));
    auto local = [&](long long n, int i, const char* what) {
        if (n < src_first || n >= (long long)src_first + nsrc)
            refuse("plan entry " + std::to_string(i) + ": " + what + " " + std::to_string(n) + " is outside the batch [" + std::to_string(src_first) + ", " +
                   std::to_string(src_first + nsrc) + ")");
        return (int)(n - src_first);
    };
    for (int i = 0; i < nout; ++i) {
        const AmtGpuRenderFrame& f = plan[i];
        if (f.kind < AMTGPU_RENDER_WEAVE || f.kind > AMTGPU_RENDER_BOB_BOTTOM) refuse("plan entry " + std::to_string(i) + ": kind outside 0..2");
        if (f.kind != AMTGPU_RENDER_WEAVE && f.top != f.bottom) refuse("plan entry " + std::to_string(i) + ": a BOB entry needs top == bottom");
        if (adaptive) {
            // both bobs read both neighbours of n, wherever the clip has them
            RenderAdaptiveEntry& e = aentries[(size_t)i];
            e.kind = f.kind;
            e.top = local(f.top, i, "top frame");
            e.bottom = local(f.bottom, i, "bottom frame");
            e.prev = e.next = e.top;
            if (f.kind != AMTGPU_RENDER_WEAVE && f.top >= 1) e.prev = local((long long)f.top - 1, i, "the neighbour frame");
            if (f.kind != AMTGPU_RENDER_WEAVE && (long long)f.top + 1 < clip_frames) e.next = local((long long)f.top + 1, i, "the neighbour frame");
            continue;
        }
        RenderEntry& e = entries[(size_t)i];
        e.kind = f.kind;
        e.top = local(f.top, i, "top frame");
        e.bottom = local(f.bottom, i, "bottom frame");
        e.other = e.top;
        if (thresh >= 0 && f.kind == AMTGPU_RENDER_BOB_TOP && f.top >= 1) e.other = local((long long)f.top - 1, i, "the temporal neighbour");
        if (thresh >= 0 && f.kind == AMTGPU_RENDER_BOB_BOTTOM && (long long)f.top + 1 < clip_frames) e.other = local((long long)f.top + 1, i, "the temporal neighbour");
    }

    const PlaneBytes sb = kPair.bytes(s, width, height), db = kPair.bytes(d, width, height);
    kPair.disjoint(sb, nsrc, db, nout);
    RenderArgs a;
    pair_args(a, sb, db);
    a.rowY = sb.row[0]; a.rowUV = sb.row[1];
    a.H = height; a.HUV = sb.rows[1];
    a.es = s.es;
    a.thresh = thresh < 0 ? -1 : std::min(thresh, maxv);
    a.vec = render_vec16(sb.luma(), sb.chroma(), db.luma(), db.chroma());
    c->bind();
    if (adaptive) {
        DevBuf<RenderAdaptiveEntry> dplan;
        dplan.upload(aentries, c->stream);
        const bool planes = !s.interleaved && !s.shift;                              // planar LSB: the planar kernel, as before
        const int sp_ = c->prof_begin(planes ? "kfm_render_adaptive_kernel" : "kfm_render_adaptive_surfaces_kernel");
        AMT_HIP(planes ? launch_kfm_render_adaptive(c->stream, a, dplan.get(), nout)
                       : launch_kfm_render_adaptive_surfaces(c->stream, a, s.interleaved, s.shift, dplan.get(), nout));
        c->prof_end(sp_);
        AMT_HIP(hipStreamSynchronize(c->stream));      // the plan's device copy dies with this call
        return;
    }
    DevBuf<RenderEntry> dplan;
    dplan.upload(entries, c->stream);
    const bool planes = !s.interleaved && !s.shift;                                  // planar LSB: the plain kernel, as before
    const int sp_ = c->prof_begin(planes ? "kfm_render_kernel" : "kfm_render_surfaces_kernel");
    AMT_HIP(planes ? launch_kfm_render(c->stream, a, dplan.get(), nout) : launch_kfm_render_surfaces(c->stream, a, s.interleaved, s.shift, dplan.get(), nout));
    c->prof_end(sp_);
    AMT_HIP(hipStreamSynchronize(c->stream));          // the plan's device copy dies with this call
}
} // namespace

extern "C" {

int amtgpu_kfm_render_plan(const uint8_t* cadence, const uint8_t* phase, int nframes, AmtGpuRenderFrame* out, int cap, int* nout)
{
    try {
        if (nframes < 0 || (nframes > 0 && (!cadence || !phase))) return 0;
        const std::vector<RenderFrame> p = cadence_render_plan(cadence, phase, nframes);
        if (nout) *nout = (int)p.size();
        if ((int)p.size() > cap) return 0;
        if (!p.empty() && !out) return 0;
        for (size_t i = 0; i < p.size(); ++i) out[i] = AmtGpuRenderFrame{p[i].kind, p[i].top, p[i].bottom, p[i].ticks};
        return 1;
    } catch (...) { return 0; }
}

int amtgpu_kfm_render(AmtGpuContext* c, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height,
                      const AmtGpuRenderFrame* plan, int nout, int thresh, const AmtGpuSurfaces* dst)
{
    if (!c) return 0;
    return guard(c, [&] { render(c, src, src_first, nsrc, clip_frames, width, height, plan, nout, AMTGPU_DEINT_LINE, thresh, dst); });
}

int amtgpu_kfm_render_deint(AmtGpuContext* c, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height,
                            const AmtGpuRenderFrame* plan, int nout, int deint, int thresh, const AmtGpuSurfaces* dst)
{
    if (!c) return 0;
    return guard(c, [&] { render(c, src, src_first, nsrc, clip_frames, width, height, plan, nout, deint, thresh, dst); });
}

int amtgpu_kfm_render_deint_surfaces(AmtGpuContext* c, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height,
                                     const AmtGpuRenderFrame* plan, int nout, int deint, int thresh, const AmtGpuSurfaces* dst)
{
    if (!c) return 0;
    return guard(c, [&] { render(c, src, src_first, nsrc, clip_frames, width, height, plan, nout, deint, thresh, dst, true); });
}

} // extern "C"
