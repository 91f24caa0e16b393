// amt_gpu_resize.hip -- C ABI part 7: the resize in front of the temporal NR in the server's chain (BlackmanResize, Misc.cs:1423) over
// frames resident in HBM ("parity unpinned").  The object holds the four programs (luma and chroma, horizontal and
// vertical: resize_plan.hpp) on the host and on the device, and the intermediate of the horizontal stage, which is bounded by
// max_scratch_bytes and not by the clip: a call works through its frames in rounds.  Two entry points over one set of argument checks:
// amtgpu_resize_run takes planar LSB planes and nothing else; amtgpu_resize_run_surfaces takes every pair of descriptors in kind and runs
// the rule on samples (container >> shift in, result << shift out).
#include "build_knobs.h"
#include "../../include/amt_gpu.h"

#include <memory>
#include <string>

#include "api_common.hpp"
#include "plane_pair.hpp"
#include "resize_plan.hpp"

using namespace amt;

struct AmtGpuResize {
    AmtGpuContext* ctx;
    int src_w, src_h, dst_w, dst_h, bits;
    ResizeProgram prog[2][2];                  // [plane: luma, chroma][axis: horizontal, vertical]
    DevBuf<int> dTables;                       // the four programs' start and coeff, one behind the other
    ResizeProgramDev dprog[2][2];
    int cpw[2];                                // resize_columns_per_wave of the two horizontal programs
    int pair_cpw;                              // resize_pair_columns_per_wave of the chroma one, for interleaved surfaces (the object's bits
                                               // fix its container size); 0: an interleaved chroma row cannot be staged, planar ones can
    int mid_pitch[2];                          // bytes between the intermediate's rows: the row rounded up to 16
    size_t mid_plane[2], mid_frame;            // bytes of one frame's luma / one chroma plane of the intermediate, and of all three
    int round_frames;                          // frames whose intermediates fit max_scratch_bytes
    DevBuf<uint8_t> dMid;
};

namespace {
const PlanePairRule& kPair = kResizePair;
const char* const kWho = kPair.who;

[[noreturn]] void refuse(const std::string& what) { throw std::runtime_error(std::string(kWho) + " " + what); }

AmtGpuResize* resize_create(AmtGpuContext* c, int src_w, int src_h, int dst_w, int dst_h, int bits, int kernel, int taps, int64_t max_scratch_bytes)
{
    if (bits < 8 || bits > 16) refuse("bits must be 8..16");
    if (src_w <= 0 || src_h <= 0 || dst_w <= 0 || dst_h <= 0 || ((src_w | src_h | dst_w | dst_h) & 1)) refuse("all four sizes must be even and positive (4:2:0)");
    if (src_w > 32768 || src_h > 32768 || dst_w > 32768 || dst_h > 32768) refuse("sizes above 32768 are not supported");
    if (kernel != AMTGPU_RESIZE_BLACKMAN && kernel != AMTGPU_RESIZE_LANCZOS && kernel != AMTGPU_RESIZE_BILINEAR)
        refuse("kernel must be AMTGPU_RESIZE_BLACKMAN, _LANCZOS or _BILINEAR");
    if (taps > 64) refuse("taps must be at most 64");
    if (max_scratch_bytes <= 0) max_scratch_bytes = AMTGPU_RESIZE_DEFAULT_SCRATCH_BYTES;
    std::unique_ptr<AmtGpuResize> r(new AmtGpuResize{});
    r->ctx = c; r->src_w = src_w; r->src_h = src_h; r->dst_w = dst_w; r->dst_h = dst_h; r->bits = bits;
    const int es = sample_bytes(bits);
    std::vector<int> tables;
    size_t at[2][2][2];
    for (int p = 0; p < 2; ++p)
        for (int ax = 0; ax < 2; ++ax) {
            const int S = (ax ? src_h : src_w) >> p, D = (ax ? dst_h : dst_w) >> p;
            ResizeProgram& g = r->prog[p][ax];
            g = resize_program(S, D, kernel, taps);
            if (!resize_program_fits_int32(g, bits))
                refuse(std::string("the ") + (p ? "chroma" : "luma") + (ax ? " vertical" : " horizontal") + " program's sums leave the int32 accumulator at " +
                       std::to_string(bits) + " bits");
            at[p][ax][0] = tables.size(); tables.insert(tables.end(), g.start.begin(), g.start.end());
            at[p][ax][1] = tables.size(); tables.insert(tables.end(), g.coeff.begin(), g.coeff.end());
        }
    for (int p = 0; p < 2; ++p) {
        const ResizeProgram& g = r->prog[p][0];
        r->cpw[p] = resize_columns_per_wave(g.start.data(), g.D, g.K, es);
        if (!r->cpw[p])
            refuse("the horizontal window of " + std::to_string(g.K) + " samples does not fit a wave's staging region (" +
                   std::to_string((kResizeRegionBytes - kResizeRegionSlack) / es) + " samples): the ratio is too small");
        if (p) r->pair_cpw = resize_pair_columns_per_wave(g.start.data(), g.D, g.K, es);
        r->mid_pitch[p] = ((dst_w >> p) * es + 15) & ~15;
        r->mid_plane[p] = (size_t)r->mid_pitch[p] * (size_t)(src_h >> p);
    }
    r->mid_frame = r->mid_plane[0] + 2 * r->mid_plane[1];
    if ((uint64_t)max_scratch_bytes < r->mid_frame)
        refuse("max_scratch_bytes " + std::to_string(max_scratch_bytes) + " is below one frame's intermediate of " + std::to_string(r->mid_frame) + " bytes");
    r->round_frames = (int)std::min<uint64_t>((uint64_t)max_scratch_bytes / r->mid_frame, 65535);
    c->bind();
    r->dTables.upload(tables, c->stream);
    for (int p = 0; p < 2; ++p)
        for (int ax = 0; ax < 2; ++ax) {
            const ResizeProgram& g = r->prog[p][ax];
            r->dprog[p][ax] = ResizeProgramDev{r->dTables.get() + at[p][ax][0], r->dTables.get() + at[p][ax][1], g.S, g.D, g.K, 0};
        }
    return r.release();
}

// both entry points: any_layout is amtgpu_resize_run_surfaces, which takes every pair in kind
void resize_run(AmtGpuResize* r, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes, bool any_layout)
{
    AmtGpuContext* c = r->ctx;
    if (nframes < 0) refuse("negative frame count");
    if (nframes == 0) return;
    // the source/destination rule (plane_pair.hpp)
    const FrameBatch s = kPair.side("source", src, surface_batch(src, kWho), r->src_w, any_layout, r->bits),
                     t = kPair.side("destination", dst, surface_batch(dst, kWho), r->dst_w, any_layout, r->bits);
    kPair.in_kind(s, t);
    const int es = s.es, il = s.interleaved;
    const bool planes = !il && !s.shift;                                               // planar LSB: the planar kernels, as before
    if (il && !r->pair_cpw)
        refuse("the interleaved chroma window of " + std::to_string(r->prog[1][0].K) + " pairs does not fit a wave's staging region (" +
               std::to_string((kResizeRegionBytes - kResizePairSlack) / (2 * es)) + " pairs): the ratio is too small for interleaved surfaces");
    const PlaneBytes sb = kPair.bytes(s, r->src_w, r->src_h), tb = kPair.bytes(t, r->dst_w, r->dst_h);
    kPair.disjoint(sb, nframes, tb, nframes);

    c->bind();
    const int round = std::min(r->round_frames, nframes);
    const size_t need = r->mid_frame * (size_t)round;
    if (r->dMid.size() < need) r->dMid.alloc(need);      // (hipFree waits for the kernels that still use the old intermediate)
    // one round's intermediate: [round] luma planes, then [round] U planes, then [round] V planes -- or, interleaved, [round] UV planes of
    // the luma pitch, which is at most two chroma pitches: a frame's intermediate is no larger than the planar one
    const int mid_pitch[2] = {r->mid_pitch[0], il ? r->mid_pitch[0] : r->mid_pitch[1]};
    const size_t mid_plane[2] = {r->mid_plane[0], il ? (size_t)r->mid_pitch[0] * (size_t)(r->src_h / 2) : r->mid_plane[1]};
    uint8_t* const mid[3] = {r->dMid.get(), r->dMid.get() + mid_plane[0] * round, il ? nullptr : r->dMid.get() + (mid_plane[0] + mid_plane[1]) * round};
    const RowsAt midY{lane_addr(mid[0]), 0, (long long)mid_plane[0], mid_pitch[0]}, midUV{lane_addr(mid[1]), lane_addr(mid[2]), (long long)mid_plane[1], mid_pitch[1]};
    ResizeStageArgs h{}, v{};
    h.es = v.es = es;
    h.maxv = v.maxv = (1 << r->bits) - 1;
    h.vec = v.vec = planes ? resize_vec16(sb.luma(), sb.chroma(), midY, midUV, tb.luma(), tb.chroma())
                           : resize_surface_vec16(sb.luma(), sb.chroma(), midY, midUV, tb.luma(), tb.chroma());
    for (int k = 0; k < 2; ++k) {
        h.prog[k] = r->dprog[k][0]; v.prog[k] = r->dprog[k][1];
        h.lines[k] = sb.rows[k]; v.lines[k] = tb.row[k] / es;
        h.cpw[k] = k && il ? r->pair_cpw : r->cpw[k]; v.cpw[k] = 0;
    }
    for (int first = 0; first < nframes; first += round) {
        const int n = std::min(round, nframes - first);
        for (int p = 0; p < sb.nplanes; ++p) {
            const int k = p ? 1 : 0;
            h.plane[p] = ResizePlaneArgs{(const uint8_t*)sb.p[p] + first * sb.stride[k], mid[p], sb.stride[k], (long long)mid_plane[k], sb.pitch[k], mid_pitch[k]};
            v.plane[p] = ResizePlaneArgs{mid[p], (uint8_t*)tb.p[p] + first * tb.stride[k], (long long)mid_plane[k], tb.stride[k], mid_pitch[k], tb.pitch[k]};
        }
        const int s1 = c->prof_begin(planes ? "resize_h_kernel" : "resize_surface_h_kernel");
        AMT_HIP(planes ? launch_resize_h(c->stream, h, n) : launch_resize_surfaces_h(c->stream, h, il, s.shift, n));
        c->prof_end(s1);
        const int s2 = c->prof_begin(planes ? "resize_v_kernel" : "resize_surface_v_kernel");
        AMT_HIP(planes ? launch_resize_v(c->stream, v, n) : launch_resize_surfaces_v(c->stream, v, il, s.shift, n));
        c->prof_end(s2);
    }
    AMT_HIP(hipStreamSynchronize(c->stream));            // as amtgpu_temporal_nr: dst is ready when the call returns
}

void resize_get_program(AmtGpuResize* r, int plane, int axis, int* K, int* start, int* coeff)
{
    if (plane < 0 || plane > 1 || axis < 0 || axis > 1) refuse("plane is 0 (luma) or 1 (chroma), axis 0 (horizontal) or 1 (vertical)");
    const ResizeProgram& g = r->prog[plane][axis];
    if (K) *K = g.K;
    if (start) std::copy(g.start.begin(), g.start.end(), start);
    if (coeff) std::copy(g.coeff.begin(), g.coeff.end(), coeff);
}
} // namespace

extern "C" {

AmtGpuResize* amtgpu_resize_create(AmtGpuContext* c, int src_w, int src_h, int dst_w, int dst_h, int bits, int kernel, int taps, int64_t max_scratch_bytes)
{
    if (!c) return nullptr;
    AmtGpuResize* r = nullptr;
    guard(c, [&] { r = resize_create(c, src_w, src_h, dst_w, dst_h, bits, kernel, taps, max_scratch_bytes); });
    return r;
}

void amtgpu_resize_destroy(AmtGpuResize* r) { delete r; }

int amtgpu_resize_run(AmtGpuResize* r, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes)
{
    if (!r) return 0;
    return guard(r->ctx, [&] { resize_run(r, src, dst, nframes, false); });
}

int amtgpu_resize_run_surfaces(AmtGpuResize* r, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes)
{
    if (!r) return 0;
    return guard(r->ctx, [&] { resize_run(r, src, dst, nframes, true); });
}

int amtgpu_resize_get_program(AmtGpuResize* r, int plane, int axis, int* K, int* start, int* coeff)
{
    if (!r) return 0;
    return guard(r->ctx, [&] { resize_get_program(r, plane, axis, K, start, coeff); });
}

} // extern "C"
