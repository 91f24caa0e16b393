// logofind_msb_kernels.hip -- the logo finder's sums (logofind_kernels.hip) over MSB-aligned Y planes, as decoders hand them out (P010 /
// P012: the sample in the high bits of a 16-bit container): every sample is container >> shift, one v_pk_lshrrev_b16 per loaded dword, then
// the plain kernel's arithmetic.  The template is logofind_body.h; this instantiation has a file of its own so that the plain kernels are compiled
// without it: their device code is the same bytes whether or not this file exists or changes.
// Entered through launch_logofind, which hands batches with a shift on to the launcher below (declared in logofind_body.h).
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "kernels.hpp"
#include "logofind_body.h"

namespace amt {

// bits: the depth of the shifted samples (9..16), which is what bounds the uint32 partials (logofind_launch_cap)
hipError_t launch_logofind_msb(hipStream_t st, int bits, const FrameBatch& b, int W, int H, int nframes, int num_cus, unsigned long long* dS1,
                               unsigned long long* dSM)
{
    if (nframes <= 0) return hipSuccess;
    if (bits <= 8 || bits > 16 || b.shift != 16 - bits || b.es != 2 || nframes > logofind_launch_cap(bits)) return hipErrorInvalidValue;
    if ((long long)H * b.pitchY * 2 >= (1LL << 31)) return hipErrorInvalidValue;       // 32-bit buffer offsets within a frame
    const LfGrid g = logofind_grid(b.pitchY, W, H, nframes, num_cus);
    dim3 grid((unsigned)g.tiles, (unsigned)g.slices), block(64);
    if (g.buf)
        hipLaunchKernelGGL((logofind_kernel<2, true, true>), grid, block, 0, st, (const uint8_t*)b.Y, b.strideY, b.pitchY * 2, W, H, nframes,
                           g.slice_frames, g.col_waves, dS1, dSM, b.shift);
    else
        hipLaunchKernelGGL((logofind_kernel<2, false, true>), grid, block, 0, st, (const uint8_t*)b.Y, b.strideY, b.pitchY * 2, W, H, nframes,
                           g.slice_frames, g.col_waves, dS1, dSM, b.shift);
    return hipGetLastError();
}

} // namespace amt
