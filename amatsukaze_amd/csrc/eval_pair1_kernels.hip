// eval_pair1_kernels.hip -- the one-unit form of the scan's two-fade evaluation (eval_pair_kernels.hip has the kernel's story, eval_pair_body.h
// its body): for engines whose logos all have a single-pass plan (eval_tiles.hpp kTileCutUnits, chosen in EvalEngine::ensure_tiles).  A tile
// of such a plan lists the at most 64 staging units that some window of its pixels reads -- about four fifths of the bounding box on a
// logo's strokes -- so a lane holds one unit, a request is three raw loads, and no tile is staged in two passes.  Same arithmetic on the
// same samples in the same order: the records are the bits the two-unit form gives.
#include "build_knobs.h"
#include "eval_pair_body.h"

namespace amt {

template <typename pix_t>
__global__ __launch_bounds__(kPairThreads) AMT_PAIR_OCC_ATTR
void logo_eval_pair1_kernel(const PairLaunch A) { logo_eval_pair_body<pix_t, true, true>(A); }
template <typename pix_t>
__global__ __launch_bounds__(kPairThreads) AMT_PAIR_OCC_ATTR
void logo_eval_pair1_ldexp_kernel(const PairLaunch A) { logo_eval_pair_body<pix_t, false, true>(A); }

// dtls: every logo's TileLogoDev::units is set (a single-pass plan); ldexp_form as in launch_logo_eval_pair
hipError_t launch_logo_eval_pair1(hipStream_t st, int bits, const EvalLogoDev* dlogos, const TileLogoDev* dtls, int nlogos,
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
        if (bits <= 8) hipLaunchKernelGGL(logo_eval_pair1_ldexp_kernel<uint8_t>, grid, dim3(kPairThreads), lds, st, A);
        else hipLaunchKernelGGL(logo_eval_pair1_ldexp_kernel<uint16_t>, grid, dim3(kPairThreads), lds, st, A);
    } else {
        if (bits <= 8) hipLaunchKernelGGL(logo_eval_pair1_kernel<uint8_t>, grid, dim3(kPairThreads), lds, st, A);
        else hipLaunchKernelGGL(logo_eval_pair1_kernel<uint16_t>, grid, dim3(kPairThreads), lds, st, A);
    }
    return hipGetLastError();
}

} // namespace amt
