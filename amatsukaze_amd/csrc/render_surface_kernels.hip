// render_surface_kernels.hip -- the cadence renderer (render_kernels.hip) on decoder surfaces where they lie, source
// and destination in kind.  Interleaved chroma (NV12 and its 16-bit kin): the UV plane is walked as ONE plane of H / 2 rows of `width`
// containers -- the rule is vertical and temporal only, so a U and a V container each meet only their own column of the rows above, below
// and beside them, and the result is the interleave of the planar result.  MSB-aligned 16-bit containers (P010 / P012, planar or
// interleaved; s = 16 - bits): a copied row is moved as stored, low bits included; an interpolated row is computed on container >> s, one
// v_pk_lshrrev_b16 per loaded dword before any arithmetic, then the planar kernel's packed mean and select (render_body.h), then one
// v_pk_lshlrev_b16, so its low bits are zero.  The shape is the planar kernel's: one wave per output row, 16 bytes per lane where
// everything is 16-byte aligned, an interpolated row's 2 (4) loads issued together; no LDS, no atomics, no scratch.  These instantiations
// have a file of their own so that the planar LSB kernels are compiled without them.  The row walk below repeats kfm_render_kernel's:
// called from one shared function the four planar kernels compiled to other instruction streams (a reversed compare and branch with the
// arguments by value, scratch with them by reference), and they are to stay exactly as they were.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"
#include "render_body.h"

namespace amt {

// nuv: chroma planes walked behind the H luma rows (1: the interleaved UV plane at srcU / dstU, a.rowUV = width * es bytes; 2: U rows, then
// V rows).  VEC: every plane base, stride and pitch is a multiple of 16 bytes.  MSB: samples are containers >> s
template <int ES, bool VEC, bool MSB>
__global__ __launch_bounds__(256)
void kfm_render_surfaces_kernel(RenderArgs a, const RenderEntry* __restrict__ plan, int row_blocks, int nuv, int s)
{
    const int frame = blockIdx.x / row_blocks, rb = blockIdx.x - frame * row_blocks;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const RenderEntry e = plan[frame];
    const int nrows = a.H + nuv * a.HUV;
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
            // a woven or kept row, as stored: even rows from top, odd rows from bottom (the same picture for the bobs)
            const uint8_t* src = srow(odd ? e.bottom : e.top, y);
            if constexpr (VEC) {
                for (int x = lane * 16; x + 16 <= nb; x += 64 * 16) *reinterpret_cast<uint4*>(d + x) = *reinterpret_cast<const uint4*>(src + x);
                for (int k = (nb & ~15) + lane; k < nb; k += 64) d[k] = src[k];
            } else {
                for (int x = lane; x < nb; x += 64) d[x] = src[x];
            }
        } else {
            const int yu = y > 0 ? y - 1 : y + 1, yd = y + 1 < h ? y + 1 : y - 1;      // (h >= 2: one of the two neighbours always exists)
            const uint8_t *up = srow(e.top, yu), *dn = srow(e.top, yd);
            if (a.thresh >= 0) render_fill_row<ES, VEC, true, MSB>(d, up, dn, srow(e.top, y), srow(e.other, y), nb, a.thresh, lane, s);
            else render_fill_row<ES, VEC, false, MSB>(d, up, dn, nullptr, nullptr, nb, 0, lane, s);
        }
    }
}

hipError_t launch_kfm_render_surfaces(hipStream_t st, const RenderArgs& a, int interleaved, int shift, const RenderEntry* dplan, int nout)
{
    if (nout <= 0) return hipSuccess;
    if ((a.es != 1 && a.es != 2) || shift < 0 || shift > 7 || (shift && a.es != 2)) return hipErrorInvalidValue;
    const int nuv = interleaved ? 1 : 2;
    const int nrows = a.H + nuv * a.HUV;
    const long long row_blocks = (nrows + kRenderRows - 1) / kRenderRows;
    if (row_blocks * nout > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    dim3 grid((unsigned)(row_blocks * nout)), block(256);
#define AMT_RENDER_LAUNCH(ES, VEC, MSB) \
    hipLaunchKernelGGL((kfm_render_surfaces_kernel<ES, VEC, MSB>), grid, block, 0, st, a, dplan, (int)row_blocks, nuv, shift)
    if (shift) { if (a.vec) AMT_RENDER_LAUNCH(2, true, true); else AMT_RENDER_LAUNCH(2, false, true); }
    else if (a.es == 1) { if (a.vec) AMT_RENDER_LAUNCH(1, true, false); else AMT_RENDER_LAUNCH(1, false, false); }
    else { if (a.vec) AMT_RENDER_LAUNCH(2, true, false); else AMT_RENDER_LAUNCH(2, false, false); }
#undef AMT_RENDER_LAUNCH
    return hipGetLastError();
}

} // namespace amt
