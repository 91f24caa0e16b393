// logofind_kernels.hip -- whole-frame edge-persistence sums of the automatic logo finder (self-specified).
//
// Per pixel, over every frame offered (Y plane only, 8..16-bit samples):
//   S1[y][x] += Y[y][x]                                                         every pixel
//   SM[y][x] += |Y[y][x+1] - Y[y][x-1]| + |Y[y+1][x] - Y[y-1][x]|               1 <= x <= W-2, 1 <= y <= H-2 (0 on the outer ring)
// The summed signed gradient is linear in the frames and comes from S1 on the host (logo_find.cpp); only the magnitudes need a pass over
// every frame.  Both sums are integers: exact, independent of frame order, batch split and GPU count.
//
// Streaming reduction in the style of frame_stats_kernel (stats_kernels.hip): a wave owns a tile of kRows rows by 62 lane columns of
// 4 samples and walks the frames of its slice.  Lanes 1..62 own pixels; lanes 0 and 63 only load the columns either side of the span,
// whose samples reach the owners through DPP (wave_shr:1 / wave_shl:1) -- those two columns are the only samples read twice.  The rows
// above and below the tile come from the lane's own R+2 row loads.  The per-pixel partials sit in VGPRs as uint32 across the frames of
// the launch (the host caps a launch at floor((2^31-1) / (2*maxv)) frames) and are added into the int64 accumulators once per launch
// with 64-bit vector atomics: the frames of a launch are dealt to `gridDim.y` slices so that small frames still fill the device.
//
// Per pixel and frame the vector ALU does one add (S1) and two v_sad_u16 on unpacked samples (|a - b| + acc in one instruction, SM).
// A packed 16-bit form (v_pk_max_u16 / v_pk_min_u16 / v_pk_sub_u16 on sample pairs, then widening adds into 32-bit partials) costs
// 2.5 instructions per pair and term against the two of the unpacked v_sad_u16 -- see DESIGN.md 6b.  No LDS, no scratch, no MFMA; every
// memory instruction is a vector one.
//
// The kernel template itself is in logofind_body.h: this file instantiates its four plain forms ({8, 16}-bit samples x {buffer,
// sample-wise} loads); the form for MSB-aligned 16-bit containers is instantiated in logofind_msb_kernels.hip.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "kernels.hpp"
#include "logofind_body.h"

namespace amt {

long long logofind_launch_cap(int bits) { return (long long)((2147483647LL) / (2LL * ((1LL << bits) - 1))); }

hipError_t launch_logofind(hipStream_t st, int bits, const FrameBatch& b, int W, int H, int nframes, int num_cus, unsigned long long* dS1,
                           unsigned long long* dSM)
{
    if (nframes <= 0) return hipSuccess;
    if (b.shift) return launch_logofind_msb(st, bits, b, W, H, nframes, num_cus, dS1, dSM);
    if (nframes > logofind_launch_cap(bits)) return hipErrorInvalidValue;
    const int es = bits <= 8 ? 1 : 2;
    if (b.es != es) return hipErrorInvalidValue;
    if ((long long)H * b.pitchY * es >= (1LL << 31)) return hipErrorInvalidValue;      // 32-bit buffer offsets within a frame
    const LfGrid g = logofind_grid(b.pitchY, W, H, nframes, num_cus);
    const bool buf = g.buf;
    dim3 grid((unsigned)g.tiles, (unsigned)g.slices), block(64);
#define AMT_LF_LAUNCH(E, BF)                                                                                                   \
    hipLaunchKernelGGL((logofind_kernel<E, BF, false>), grid, block, 0, st, (const uint8_t*)b.Y, b.strideY, b.pitchY * es, W, H, nframes, \
                       g.slice_frames, g.col_waves, dS1, dSM, 0)
    if (es == 1) { if (buf) AMT_LF_LAUNCH(1, true); else AMT_LF_LAUNCH(1, false); }
    else { if (buf) AMT_LF_LAUNCH(2, true); else AMT_LF_LAUNCH(2, false); }
#undef AMT_LF_LAUNCH
    return hipGetLastError();
}

} // namespace amt
