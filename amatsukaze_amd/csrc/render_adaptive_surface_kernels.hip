// render_adaptive_surface_kernels.hip -- the adaptive bob (render_adaptive_kernels.hip; DESIGN.md section 6d, "the adaptive rule") on
// decoder surfaces where they lie, source and destination in kind.  The result is defined on samples: de-interleave UV into U and V, each
// its own plane of width / 2 columns with its own column clamp; take container >> s; apply the planar rule per plane; store an
// interpolated container as result << s, its low bits zero; re-interleave.  Every copied row (all rows of a WEAVE, the kept rows of a bob)
// is moved as stored, low bits included.  Unlike the line rule this one looks sideways (columns x - 3 .. x + 3), so an interleaved UV row
// cannot be walked as one plane of `width` containers: a U container's neighbours are two containers away and the clamp is per component
// (render_adaptive_body.h, STEP 2).  One launch per call: in an interleaved form the luma rows run the unit-step row function and the UV
// rows the step-2 one under a wave-uniform branch on the row's plane.  The shape is the planar kernel's: one wave per output row, four
// rows per workgroup, no row loop, 16 bytes per lane where everything is 16-byte aligned, the 12 row segments of a span loaded before the
// first use, the neighbours' containers over DPP wave shifts; no LDS, no atomics, no scratch.  The row walk below repeats
// kfm_render_adaptive_kernel's, as render_surface_kernels.hip repeats kfm_render_kernel's and for the same reason: the four planar
// kernels are to stay exactly as they were.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"
#include "render_adaptive_body.h"

namespace amt {

// IL: the chroma behind the H luma rows is the one interleaved UV plane at srcU / dstU (a.rowUV = width * es bytes), else U rows, then V
// rows.  VEC: every plane base, stride and pitch is a multiple of 16 bytes.  MSB: samples are containers >> s.
// The 16-bit forms are compiled for five waves per SIMD (at most 96 VGPRs; their vector forms take 84 to 89, no spills): left to itself
// the compiler takes 97 to 104 for them, four waves, against the six of the planar 16-bit kernel this is measured against, and P010 at
// 1080p ran 8 % slower for it.  Six waves (80 VGPRs) spill in the interleaved forms.  The 8-bit forms keep the
// planar kernel's four
template <int ES, bool VEC, bool MSB, bool IL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ES == 2 ? 5 : 4, 8)))
void kfm_render_adaptive_surfaces_kernel(RenderArgs a, const RenderAdaptiveEntry* __restrict__ plan, int row_blocks, int s)
{
    const int frame = blockIdx.x / row_blocks, rb = blockIdx.x - frame * row_blocks;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const RenderAdaptiveEntry e = plan[frame];
    const int nrows = a.H + (IL ? 1 : 2) * a.HUV;
    const int r = rb * kAdpRows + wave;                                                  // one row per wave, no loop: nothing but the row stays live
    if (r < nrows) {
        int pl, y;
        if (r < a.H) { pl = 0; y = r; } else if (r < a.H + a.HUV) { pl = 1; y = r - a.H; } else { pl = 2; y = r - a.H - a.HUV; }
        const uint8_t* sp = pl == 0 ? a.srcY : pl == 1 ? a.srcU : a.srcV;
        uint8_t* dp = pl == 0 ? a.dstY : pl == 1 ? a.dstU : a.dstV;
        const long long ss = pl == 0 ? a.src_strideY : a.src_strideUV, ds = pl == 0 ? a.dst_strideY : a.dst_strideUV;
        const int spitch = pl == 0 ? a.src_pitchY : a.src_pitchUV, dpitch = pl == 0 ? a.dst_pitchY : a.dst_pitchUV;
        const int nb = pl == 0 ? a.rowY : a.rowUV, h = pl == 0 ? a.H : a.HUV;
        auto srow = [&](int pic, int yy) { return sp + (long long)pic * ss + (long long)yy * spitch; };
        uint8_t* d = dp + (long long)frame * ds + (long long)y * dpitch;
        const int odd = y & 1;
        if (e.kind == 0 || odd == (e.kind == 2)) {
            // a woven or kept row, as stored: even rows from top, odd rows from bottom (the same picture for the bobs)
            const uint8_t* src = srow(odd ? e.bottom : e.top, y);
            if constexpr (VEC) {
                for (int x = lane * 16; x + 16 <= nb; x += 64 * 16) *reinterpret_cast<uint4*>(d + x) = *reinterpret_cast<const uint4*>(src + x);
                for (int k = (nb & ~15) + lane; k < nb; k += 64) d[k] = src[k];
            } else {
                for (int x = lane; x < nb; x += 64) d[x] = src[x];
            }
        } else {
            // (h >= 2: one of the rows y - 1, y + 1 always exists)
            const int y1m = y > 0 ? y - 1 : y + 1, y1p = y + 1 < h ? y + 1 : y - 1, y2m = y >= 2 ? y - 2 : y, y2p = y + 2 < h ? y + 2 : y;
            const int pa = e.kind == 1 ? e.prev : e.top, pb = e.kind == 1 ? e.top : e.next;   // the missing parity's fields before and after the kept one
            const int y0 = max(y - 2, 0);                                               // every row read lies in [y0, y0 + 4]
            auto off = [&](int yy) { return (uint32_t)((yy - y0) * spitch); };
            const AdpRows rows = {srow(e.top, y0), srow(e.prev, y0), srow(e.next, y0), srow(pa, y0), srow(pb, y0), off(y), off(y1m), off(y1p), off(y2m), off(y2p)};
            if (IL && pl != 0) adp_fill_row<ES, VEC, MSB, 2>(d, rows, nb, lane, s);     // (wave-uniform: a wave has one row)
            else adp_fill_row<ES, VEC, MSB, 1>(d, rows, nb, lane, s);
        }
    }
}

hipError_t launch_kfm_render_adaptive_surfaces(hipStream_t st, const RenderArgs& a, int interleaved, int shift, const RenderAdaptiveEntry* dplan, int nout)
{
    if (nout <= 0) return hipSuccess;
    if ((a.es != 1 && a.es != 2) || shift < 0 || shift > 7 || (shift && a.es != 2)) return hipErrorInvalidValue;
    if (!interleaved && !shift) return hipErrorInvalidValue;                             // planar LSB planes are launch_kfm_render_adaptive's
    if (interleaved && (a.rowUV & (2 * a.es - 1))) return hipErrorInvalidValue;          // a UV row is whole pairs
    const int nrows = a.H + (interleaved ? 1 : 2) * a.HUV;
    const long long row_blocks = (nrows + kAdpRows - 1) / kAdpRows;
    if (row_blocks * nout > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    dim3 grid((unsigned)(row_blocks * nout)), block(256);
#define AMT_ADP_LAUNCH(ES, VEC, MSB, IL) \
    hipLaunchKernelGGL((kfm_render_adaptive_surfaces_kernel<ES, VEC, MSB, IL>), grid, block, 0, st, a, dplan, (int)row_blocks, shift)
    if (!interleaved) { if (a.vec) AMT_ADP_LAUNCH(2, true, true, false); else AMT_ADP_LAUNCH(2, false, true, false); }
    else if (shift) { if (a.vec) AMT_ADP_LAUNCH(2, true, true, true); else AMT_ADP_LAUNCH(2, false, true, true); }
    else if (a.es == 1) { if (a.vec) AMT_ADP_LAUNCH(1, true, false, true); else AMT_ADP_LAUNCH(1, false, false, true); }
    else { if (a.vec) AMT_ADP_LAUNCH(2, true, false, true); else AMT_ADP_LAUNCH(2, false, false, true); }
#undef AMT_ADP_LAUNCH
    return hipGetLastError();
}

} // namespace amt
