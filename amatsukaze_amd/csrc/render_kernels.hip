// render_kernels.hip -- the pictures of the cadence decisions (self-specified, "parity unpinned": KFMDeint's source is not in the reference
// tree): field-matched film frames (weave) and bob-deinterlaced video fields, written straight from the source
// frames in HBM.  Per output frame one plan entry: WEAVE takes even rows from picture `top` and odd rows from picture `bottom`;
// BOB_TOP / BOB_BOTTOM keep the even / odd rows of picture n and fill each missing row y with
//     |a - b| <= thresh (and thresh >= 0) ? (a + b + 1) >> 1 : (up + dn + 1) >> 1
// up / dn = rows y - 1 / y + 1 of n (one outside the plane takes the other's value), a / b = row y of the two pictures whose field of that
// parity lies before and after the kept field in time (n - 1 and n for BOB_TOP, n and n + 1 for BOB_BOTTOM).  The rule is symmetric in a
// and b, so the plan names only the picture that is not n (`other`).  Samples are the containers as stored.
// HBM-bound like the weave it is shaped after: one wave per output row, 16 bytes per lane where everything is 16-byte aligned, an
// interpolated row's 2 (4) loads issued together, packed arithmetic; no LDS, no atomics, no scratch.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"
#include "render_body.h"

namespace amt {

// kRenderRows and the packed helpers (render_avg, render_within, render_mix, render_fill_row) are render_body.h's: one text with the
// decoder-surface kernels (render_surface_kernels.hip)

// VEC: every plane base, stride and pitch is a multiple of 16 bytes
template <int ES, bool VEC>
__global__ __launch_bounds__(256)
void kfm_render_kernel(RenderArgs a, const RenderEntry* __restrict__ plan, int row_blocks)
{
    const int frame = blockIdx.x / row_blocks, rb = blockIdx.x - frame * row_blocks;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const RenderEntry e = plan[frame];
    const int nrows = a.H + 2 * a.HUV;                                                  // Y rows, then U rows, then V rows
#pragma unroll 1
    for (int r = rb * kRenderRows + wave; r < min(nrows, (rb + 1) * kRenderRows); r += 4) {
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
            // a woven or kept row: even rows from top, odd rows from bottom (the same picture for the bobs)
            const uint8_t* s = srow(odd ? e.bottom : e.top, y);
            if constexpr (VEC) {
                for (int x = lane * 16; x + 16 <= nb; x += 64 * 16) *reinterpret_cast<uint4*>(d + x) = *reinterpret_cast<const uint4*>(s + x);
                for (int k = (nb & ~15) + lane; k < nb; k += 64) d[k] = s[k];
            } else {
                for (int x = lane; x < nb; x += 64) d[x] = s[x];
            }
        } else {
            const int yu = y > 0 ? y - 1 : y + 1, yd = y + 1 < h ? y + 1 : y - 1;      // (h >= 2: one of the two neighbours always exists)
            const uint8_t *up = srow(e.top, yu), *dn = srow(e.top, yd);
            if (a.thresh >= 0) render_fill_row<ES, VEC, true>(d, up, dn, srow(e.top, y), srow(e.other, y), nb, a.thresh, lane);
            else render_fill_row<ES, VEC, false>(d, up, dn, nullptr, nullptr, nb, 0, lane);
        }
    }
}

hipError_t launch_kfm_render(hipStream_t st, const RenderArgs& a, const RenderEntry* dplan, int nout)
{
    if (nout <= 0) return hipSuccess;
    if (a.es != 1 && a.es != 2) return hipErrorInvalidValue;
    const int nrows = a.H + 2 * a.HUV;
    const long long row_blocks = (nrows + kRenderRows - 1) / kRenderRows;
    if (row_blocks * nout > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    dim3 grid((unsigned)(row_blocks * nout)), block(256);
    if (a.es == 1 && a.vec) hipLaunchKernelGGL((kfm_render_kernel<1, true>), grid, block, 0, st, a, dplan, (int)row_blocks);
    else if (a.es == 1) hipLaunchKernelGGL((kfm_render_kernel<1, false>), grid, block, 0, st, a, dplan, (int)row_blocks);
    else if (a.vec) hipLaunchKernelGGL((kfm_render_kernel<2, true>), grid, block, 0, st, a, dplan, (int)row_blocks);
    else hipLaunchKernelGGL((kfm_render_kernel<2, false>), grid, block, 0, st, a, dplan, (int)row_blocks);
    return hipGetLastError();
}

} // namespace amt
