// stats_msb_kernels.hip -- the frame metrics (stats_kernels.hip) over MSB-aligned Y planes, as decoders hand them out (P010 / P012: the
// sample in the high bits of a 16-bit container): every sample is container >> shift, one v_pk_lshrrev_b16 per loaded dword, then the plain
// kernel's arithmetic.  The template is stats_body.h; these instantiations have a file of their own so that the plain kernels are compiled
// without them: their device code is the same bytes whether or not this file exists or changes.
// Entered through launch_frame_stats, which hands batches with a shift on to the launcher below (declared in stats_body.h).
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"
#include "stats_body.h"

namespace amt {

// bits: the depth of the shifted samples (9..15).  They are smaller than their containers, so the plain 16-bit kernel's uint32 partial sums hold.
hipError_t launch_frame_stats_msb(hipStream_t st, int bits, const FrameBatch& b, int W, int H, const void* dprevY, int nframes, unsigned long long* dout)
{
    if (nframes <= 0) return hipSuccess;
    if (bits <= 8 || bits > 15 || b.shift != 16 - bits || b.es != 2) return hipErrorInvalidValue;
    const StatGrid g = stat_grid(2, b.pitchY, W, H, nframes);
    if (!g.fits) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(dout, 0, (size_t)nframes * kStatWords * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)g.gx, (unsigned)g.gy), block(kStatThreads);
#define AMT_STATS_LAUNCH(RG, BF)                                                                                                             \
    hipLaunchKernelGGL((frame_stats_kernel<2, RG, BF, true>), grid, block, 0, st, (const uint8_t*)b.Y, b.strideY, b.pitchY * 2, g.row_bytes, H, \
                       (const uint8_t*)dprevY, nframes, g.col_groups, dout, b.shift)
    if (!g.buf) AMT_STATS_LAUNCH(true, false); else if (g.ragged) AMT_STATS_LAUNCH(true, true); else AMT_STATS_LAUNCH(false, true);
#undef AMT_STATS_LAUNCH
    return hipGetLastError();
}

} // namespace amt
