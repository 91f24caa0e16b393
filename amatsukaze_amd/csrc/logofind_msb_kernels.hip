// logofind_msb_kernels.hip -- the logo finder's sums (logofind_kernels.hip) over MSB-aligned Y planes, as decoders hand them out (P010 /
// P012: the sample in the high bits of a 16-bit container): every sample is container >> shift, one v_pk_lshrrev_b16 per loaded dword, then
// the plain kernel's arithmetic.  The template is logofind_body.h; this instantiation has a file of its own so that the plain kernels are compiled
// without it.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "kernels.hpp"
#include "logofind_body.h"

namespace amt {

// bits: the depth of the shifted samples (9..16), which is what bounds the uint32 partials (logofind_launch_cap)
hipError_t launch_logofind_msb(hipStream_t st, int bits, int shift, const void* dY, long long frame_stride, int pitch_elems, int W, int H,
                               int nframes, int num_cus, unsigned long long* dS1, unsigned long long* dSM)
{
    if (nframes <= 0) return hipSuccess;
    if (bits <= 8 || bits > 16 || shift != 16 - bits || nframes > logofind_launch_cap(bits)) return hipErrorInvalidValue;
    if ((long long)H * pitch_elems * 2 >= (1LL << 31)) return hipErrorInvalidValue;       // 32-bit buffer offsets within a frame
    const LfGrid g = logofind_grid(pitch_elems, W, H, nframes, num_cus);
    dim3 grid((unsigned)g.tiles, (unsigned)g.slices), block(64);
    if (g.buf)
        hipLaunchKernelGGL((logofind_kernel<2, true, true>), grid, block, 0, st, (const uint8_t*)dY, frame_stride, pitch_elems * 2, W, H, nframes,
                           g.slice_frames, g.col_waves, dS1, dSM, shift);
    else
        hipLaunchKernelGGL((logofind_kernel<2, false, true>), grid, block, 0, st, (const uint8_t*)dY, frame_stride, pitch_elems * 2, W, H, nframes,
                           g.slice_frames, g.col_waves, dS1, dSM, shift);
    return hipGetLastError();
}

} // namespace amt
