// render_adaptive_kernels.hip -- the cadence renderer's edge-directed, motion-adaptive bob (self-specified, "parity unpinned"; DESIGN.md
// section 6d, "the adaptive rule").  WEAVE entries and the kept rows of a bob are moved exactly as kfm_render_kernel moves them; a missing
// row y of BOB_TOP(n) / BOB_BOTTOM(n) is, per pixel and in signed integers over the containers as stored,
//     U = C[y-1], D = C[y+1], c = U[x], e = D[x]                       (C = n, P = n - 1, N = n + 1; rows and columns clamped as below)
//     d = (A[y] + B[y]) >> 1                                            ((A, B) = (P, C) for BOB_TOP, (C, N) for BOB_BOTTOM)
//     diff = max(|A[y] - B[y]| >> 1, (|P[y-1] - c| + |P[y+1] - e|) >> 1, (|N[y-1] - c| + |N[y+1] - e|) >> 1)
//     pred = (U[x+j] + D[x-j]) >> 1 for the slope j of -2..2 with the smallest three-tap score sum |U[x+j+i] - D[x-j+i]|, i = -1..1 (j = 0
//            scores one less; -1 then -2, +1 then +2 against the running score, +-2 only where +-1 improved)
//     b = (A[y-2] + B[y-2]) >> 1, f = (A[y+2] + B[y+2]) >> 1
//     diff = max(diff, min(d - e, d - c, max(b - c, f - e)), -max(d - e, d - c, min(b - c, f - e)))
//     out = pred clamped into [d - diff, d + diff]
// A row y - 1 / y + 1 outside the plane takes the other one, a row y - 2 / y + 2 outside it takes y; a column outside it takes the nearest.
// One wave per output row, 16 bytes per lane where everything is 16-byte aligned: the 12 row segments of a lane's span are loaded
// before the first use, the three containers to the left and right of a span come from the neighbouring lanes' registers (v_mov_b32_dpp
// wave_shr:1 / wave_shl:1; no LDS), and only the lanes at the seams -- lane 0, lane 63, the row's last 16-byte span -- load theirs
// container by container with the column clamp.  8-bit containers are computed two to a register in 16-bit halves (every intermediate
// lies in [-765, 765]), 16-bit containers one to a register in 32 bits (differences need 17 bits and a sign).  No LDS, no atomics, no
// scratch.  The rule's text is render_adaptive_body.h's: one text with the decoder-surface kernels (render_adaptive_surface_kernels.hip).
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"
#include "render_adaptive_body.h"

namespace amt {

// VEC: every plane base, stride and pitch is a multiple of 16 bytes
template <int ES, bool VEC>
__global__ __launch_bounds__(256)
void kfm_render_adaptive_kernel(RenderArgs a, const RenderAdaptiveEntry* __restrict__ plan, int row_blocks)
{
    const int frame = blockIdx.x / row_blocks, rb = blockIdx.x - frame * row_blocks;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const RenderAdaptiveEntry e = plan[frame];
    const int nrows = a.H + 2 * a.HUV;                                                  // Y rows, then U rows, then V rows
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
            // a woven or kept row: even rows from top, odd rows from bottom (the same picture for the bobs)
            const uint8_t* s = srow(odd ? e.bottom : e.top, y);
            if constexpr (VEC) {
                for (int x = lane * 16; x + 16 <= nb; x += 64 * 16) *reinterpret_cast<uint4*>(d + x) = *reinterpret_cast<const uint4*>(s + x);
                for (int k = (nb & ~15) + lane; k < nb; k += 64) d[k] = s[k];
            } else {
                for (int x = lane; x < nb; x += 64) d[x] = s[x];
            }
        } else {
            // (h >= 2: one of the rows y - 1, y + 1 always exists)
            const int y1m = y > 0 ? y - 1 : y + 1, y1p = y + 1 < h ? y + 1 : y - 1, y2m = y >= 2 ? y - 2 : y, y2p = y + 2 < h ? y + 2 : y;
            const int pa = e.kind == 1 ? e.prev : e.top, pb = e.kind == 1 ? e.top : e.next;   // the missing parity's fields before and after the kept one
            const int y0 = max(y - 2, 0);                                               // every row read lies in [y0, y0 + 4]
            auto off = [&](int yy) { return (uint32_t)((yy - y0) * spitch); };
            const AdpRows rows = {srow(e.top, y0), srow(e.prev, y0), srow(e.next, y0), srow(pa, y0), srow(pb, y0), off(y), off(y1m), off(y1p), off(y2m), off(y2p)};
            adp_fill_row<ES, VEC>(d, rows, nb, lane);
        }
    }
}

hipError_t launch_kfm_render_adaptive(hipStream_t st, const RenderArgs& a, const RenderAdaptiveEntry* dplan, int nout)
{
    if (nout <= 0) return hipSuccess;
    if (a.es != 1 && a.es != 2) return hipErrorInvalidValue;
    const int nrows = a.H + 2 * a.HUV;
    const long long row_blocks = (nrows + kAdpRows - 1) / kAdpRows;
    if (row_blocks * nout > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    dim3 grid((unsigned)(row_blocks * nout)), block(256);
    if (a.es == 1 && a.vec) hipLaunchKernelGGL((kfm_render_adaptive_kernel<1, true>), grid, block, 0, st, a, dplan, (int)row_blocks);
    else if (a.es == 1) hipLaunchKernelGGL((kfm_render_adaptive_kernel<1, false>), grid, block, 0, st, a, dplan, (int)row_blocks);
    else if (a.vec) hipLaunchKernelGGL((kfm_render_adaptive_kernel<2, true>), grid, block, 0, st, a, dplan, (int)row_blocks);
    else hipLaunchKernelGGL((kfm_render_adaptive_kernel<2, false>), grid, block, 0, st, a, dplan, (int)row_blocks);
    return hipGetLastError();
}

} // namespace amt
