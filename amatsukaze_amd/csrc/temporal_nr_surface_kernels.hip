// temporal_nr_surface_kernels.hip -- the temporal noise reduction (temporal_nr_body.h) on decoder surfaces where
// they lie, source and destination in kind: NV12, interleaved LSB, P010 / P012 and planar MSB.  The result is defined on samples:
// de-interleave UV into U (even containers) and V (odd containers), take container >> s, apply the planar rule, store every container
// as result << s with zero low bits, re-interleave.  Nothing is copied from the source, so low bits never survive.  It is the shared
// cell with MSB and IL as the kind asks; planar MSB keeps the planar kernel's two 8-byte chroma runs.  One launch.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"
#include "temporal_nr_body.h"

namespace amt {

// VEC: temporal_nr_surface_vec16 (lane_rule.h).  A block takes 256 consecutive cells of one output frame, as temporal_nr_kernel does
template <typename T, bool VEC, bool MSB, bool IL>
__global__ __launch_bounds__(256)
void temporal_nr_surfaces_kernel(TemporalNRArgs a, int cells_per_row, int blocks_per_frame, int s)
{
    constexpr int PX = VEC ? 16 / (int)sizeof(T) : 2;
    const int out = blockIdx.x / blocks_per_frame;
    const int cell = (blockIdx.x - out * blocks_per_frame) * 256 + threadIdx.x;
    const int cy = cell / cells_per_row, x0 = (cell - cy * cells_per_row) * PX;
    if (cy >= (a.H >> 1)) return;
    const int y0 = a.interlaced ? 2 * (cy & ~1) + (cy & 1) : 2 * cy, y1 = a.interlaced ? y0 + 2 : y0 + 1;
    const int centre = a.first + out;
    if constexpr (VEC) {
        if (x0 + PX <= a.W) { tnr_cell<T, true, MSB, IL, PX>(a, s, out, centre, y0, y1, cy, x0); return; }
#pragma unroll 1
        for (int x = x0; x < a.W; x += 2) tnr_cell<T, false, MSB, IL, 2>(a, s, out, centre, y0, y1, cy, x);
    } else {
        tnr_cell<T, false, MSB, IL, 2>(a, s, out, centre, y0, y1, cy, x0);
    }
}

hipError_t launch_temporal_nr_surfaces(hipStream_t st, const TemporalNRArgs& a, int interleaved, int shift, int nout)
{
    if (nout <= 0) return hipSuccess;
    TemporalNRGrid g;
    if (!temporal_nr_grid(a, nout, g)) return hipErrorInvalidValue;
    if (shift < 0 || shift > 7 || (shift && a.es != 2)) return hipErrorInvalidValue;
    if (!interleaved && !shift) return hipErrorInvalidValue;                             // planar LSB planes are launch_temporal_nr's
    dim3 grid(g.blocks), block(256);
#define AMT_TNRS_LAUNCH(T, VEC, MSB, IL) \
    hipLaunchKernelGGL((temporal_nr_surfaces_kernel<T, VEC, MSB, IL>), grid, block, 0, st, a, g.cells_per_row, g.blocks_per_frame, shift)
    if (!interleaved) { if (a.vec) AMT_TNRS_LAUNCH(uint16_t, true, true, false); else AMT_TNRS_LAUNCH(uint16_t, false, true, false); }
    else if (shift) { if (a.vec) AMT_TNRS_LAUNCH(uint16_t, true, true, true); else AMT_TNRS_LAUNCH(uint16_t, false, true, true); }
    else if (a.es == 1) { if (a.vec) AMT_TNRS_LAUNCH(uint8_t, true, false, true); else AMT_TNRS_LAUNCH(uint8_t, false, false, true); }
    else { if (a.vec) AMT_TNRS_LAUNCH(uint16_t, true, false, true); else AMT_TNRS_LAUNCH(uint16_t, false, false, true); }
#undef AMT_TNRS_LAUNCH
    return hipGetLastError();
}

} // namespace amt
