// eval_pair_kernels.hip -- the two-fade evaluation of LogoFrame::ScanFrame (LogoScan.hpp:1543-1568): corr0 = EvaluateLogo(fade 0)
// and corr1 = EvaluateLogo(fade 1) of every logo on every frame, in the reference's fp32 evaluation order (bit-exact records).
//
// With fade 0 the blended window  fade*bg + (1-fade)*s  (LogoScan.hpp:244-251) IS s, with fade 1 it IS bg = a*s + b*maxv
// (0*x + y == y for finite x; the host checks that every logo coefficient is finite and small enough for bg to stay below 2^30,
// and launches the generic kernel of eval_fused_kernels.hip otherwise).  So the two evaluations of a mask pixel are the SAME
// instruction stream on two operands: LDS holds {s, bg} pairs, a window element arrives as one 8-byte read, and every
// add / sub / mul of CalcCorrelation5x5_AVX's order (ComputeKernel.cpp:77-121, exact_math.h) is one packed fp32 instruction whose
// low half evaluates fade 0 and whose high half evaluates fade 1 -- no blend arithmetic, no FMA contraction
// (-ffp-contract=off), the 25 taps broadcast to both halves through op_sel.
//
// Shape (eval_tiles.hpp): workgroup = (logo, G <= 8 frames) = kTileWaves (11) evaluation waves + 1 summing wave, walking the logo's
// bands of <= 64 kTileWaves raster-consecutive mask pixels.  Within a band every evaluation wave owns a TILE: 64 of the band's mask pixels (the
// band sorted by column and dealt out 64 at a time) and the bounding box of their 5x5 windows.  The wave stages its tile for
// one frame per iteration into LDS nobody else touches -- raw samples prefetched into registers an iteration ahead, converted to
// {s, bg} with the tile's logo coefficients held in registers for the whole band -- and evaluates its pixels from it.  LDS
// operations of one wave complete in order, so nothing in an iteration needs a barrier.  The per-pixel terms go to an LDS row
// per (frame, fade) at the pixel's raster position; the waves meet ONCE PER BAND, and the last wave then adds the band's
// 2 G rows front to back -- one lane per row, the reference's order (`result += score`, LogoScan.hpp:295-315) -- while the
// others evaluate the next band into the second set of rows.
//
// The loop is bound by the NUMBER of vector instructions a wave issues (two to three waves per SIMD sustain one per ~6 cycles
// whatever their mix: profiles/r03_notes.md), so the code around the 101 packed operations of a window is kept short: raw
// bytes are blended two samples per instruction (16-bit lanes), a tile of at most 64 units is staged in one pass, every
// address that does not change within a band is kept in a register.
#include "build_knobs.h"
#include "eval_pair_body.h"

namespace amt {

template <typename pix_t>
__global__ __launch_bounds__(kPairThreads) AMT_PAIR_OCC_ATTR
void logo_eval_pair_kernel(const PairLaunch A) { logo_eval_pair_body<pix_t, true>(A); }
template <typename pix_t>
__global__ __launch_bounds__(kPairThreads) AMT_PAIR_OCC_ATTR
void logo_eval_pair_ldexp_kernel(const PairLaunch A) { logo_eval_pair_body<pix_t, false>(A); }

// ldexp_form: the engine's tables are NOT scaled (EvalEngine::ensure_tiles)
hipError_t launch_logo_eval_pair(hipStream_t st, int bits, const EvalLogoDev* dlogos, const TileLogoDev* dtls, int nlogos,
                                 const FrameBatch& luma, const int* dframe_map,
                                 int nframes, int G, float* dout, int out_frame_stride, int take_abs, int ldexp_form)
{
    PairLaunch A;
    size_t lds;
    unsigned nwg;
    const hipError_t e = pair_launch_args(A, &lds, &nwg, bits, dlogos, dtls, nlogos, luma, dframe_map, nframes, G, dout, out_frame_stride, take_abs);
    if (e != hipSuccess || nwg == 0) return e;
    dim3 grid(nwg);
    if (ldexp_form) {
        if (bits <= 8) hipLaunchKernelGGL(logo_eval_pair_ldexp_kernel<uint8_t>, grid, dim3(kPairThreads), lds, st, A);
        else hipLaunchKernelGGL(logo_eval_pair_ldexp_kernel<uint16_t>, grid, dim3(kPairThreads), lds, st, A);
    } else {
        if (bits <= 8) hipLaunchKernelGGL(logo_eval_pair_kernel<uint8_t>, grid, dim3(kPairThreads), lds, st, A);
        else hipLaunchKernelGGL(logo_eval_pair_kernel<uint16_t>, grid, dim3(kPairThreads), lds, st, A);
    }
    return hipGetLastError();
}

} // namespace amt
