// eval_pair1_duo_kernels.hip -- the one-unit form of the scan's two-fade evaluation (eval_pair1_kernels.hip; the body: eval_pair_body.h) in
// its second shape: kPairDuoWaves (7) evaluation waves + the summing wave, at most kPairDuoFrames (6) frames per workgroup, compiled for
// four waves per SIMD (the body needs 114 / 116 VGPRs), so that two workgroups of 512 threads and 75 136 B of LDS share a CU.  The
// engine takes it when tile_pair_shape (eval_tiles.hpp) says so; the plans it walks have kPairDuoWaves tiles per band.  Same arithmetic on
// the same samples in the same order as every other form: the records are the same bits.  Measurements: profiles/pair_waves_notes.md.
#include "build_knobs.h"
#include "eval_pair_body.h"

namespace amt {

constexpr int kPairDuoThreads = pair_threads(kPairDuoWaves);
#define AMT_PAIR_DUO_ATTR __launch_bounds__(kPairDuoThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))

template <typename pix_t>
__global__ AMT_PAIR_DUO_ATTR
void logo_eval_pair1_duo_kernel(const PairLaunch A) { logo_eval_pair_body<pix_t, true, true, kPairDuoWaves>(A); }
template <typename pix_t>
__global__ AMT_PAIR_DUO_ATTR
void logo_eval_pair1_duo_ldexp_kernel(const PairLaunch A) { logo_eval_pair_body<pix_t, false, true, kPairDuoWaves>(A); }

// dtls: every logo's plan is a single-pass one of kPairDuoWaves tiles per band; ldexp_form as in launch_logo_eval_pair
hipError_t launch_logo_eval_pair1_duo(hipStream_t st, int bits, const EvalLogoDev* dlogos, const TileLogoDev* dtls, int nlogos,
                                      const FrameBatch& luma, const int* dframe_map,
                                      int nframes, int G, float* dout, int out_frame_stride, int take_abs, int ldexp_form)
{
    PairLaunch A;
    size_t lds;
    unsigned nwg;
    if (G > kPairDuoFrames) return hipErrorInvalidValue;
    const hipError_t e = pair_launch_args(A, &lds, &nwg, bits, dlogos, dtls, nlogos, luma, dframe_map, nframes, G, dout, out_frame_stride, take_abs, kPairDuoWaves);
    if (e != hipSuccess || nwg == 0) return e;
    dim3 grid(nwg);
    if (ldexp_form) {
        if (bits <= 8) hipLaunchKernelGGL(logo_eval_pair1_duo_ldexp_kernel<uint8_t>, grid, dim3(kPairDuoThreads), lds, st, A);
        else hipLaunchKernelGGL(logo_eval_pair1_duo_ldexp_kernel<uint16_t>, grid, dim3(kPairDuoThreads), lds, st, A);
    } else {
        if (bits <= 8) hipLaunchKernelGGL(logo_eval_pair1_duo_kernel<uint8_t>, grid, dim3(kPairDuoThreads), lds, st, A);
        else hipLaunchKernelGGL(logo_eval_pair1_duo_kernel<uint16_t>, grid, dim3(kPairDuoThreads), lds, st, A);
    }
    return hipGetLastError();
}

} // namespace amt
