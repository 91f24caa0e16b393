// temporal_nr_kernels.hip -- the temporal noise reduction (temporal_nr_body.h) on planar LSB planes in HBM: the
// shared cell with containers that are samples and U and V planes of their own, so a vector lane's chroma is an 8-byte run of each.
// One launch.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"
#include "temporal_nr_body.h"

namespace amt {

// VEC: temporal_nr_vec16 (lane_rule.h).  A block takes 256 consecutive cells of one output frame; a cell is one lane's columns of one
// chroma row and of the two luma rows that map to it
template <typename T, bool VEC>
__global__ __launch_bounds__(256)
void temporal_nr_kernel(TemporalNRArgs a, int cells_per_row, int blocks_per_frame)
{
    constexpr int PX = VEC ? 16 / (int)sizeof(T) : 2;
    const int out = blockIdx.x / blocks_per_frame;
    const int cell = (blockIdx.x - out * blocks_per_frame) * 256 + threadIdx.x;
    const int cy = cell / cells_per_row, x0 = (cell - cy * cells_per_row) * PX;
    if (cy >= (a.H >> 1)) return;
    const int y0 = a.interlaced ? 2 * (cy & ~1) + (cy & 1) : 2 * cy, y1 = a.interlaced ? y0 + 2 : y0 + 1;
    const int centre = a.first + out;
    if constexpr (VEC) {
        if (x0 + PX <= a.W) { tnr_cell<T, true, false, false, PX>(a, 0, out, centre, y0, y1, cy, x0); return; }
#pragma unroll 1
        for (int x = x0; x < a.W; x += 2) tnr_cell<T, false, false, false, 2>(a, 0, out, centre, y0, y1, cy, x);
    } else {
        tnr_cell<T, false, false, false, 2>(a, 0, out, centre, y0, y1, cy, x0);
    }
}

hipError_t launch_temporal_nr(hipStream_t st, const TemporalNRArgs& a, int nout)
{
    if (nout <= 0) return hipSuccess;
    TemporalNRGrid g;
    if (!temporal_nr_grid(a, nout, g)) return hipErrorInvalidValue;
    dim3 grid(g.blocks), block(256);
    if (a.es == 1 && a.vec) hipLaunchKernelGGL((temporal_nr_kernel<uint8_t, true>), grid, block, 0, st, a, g.cells_per_row, g.blocks_per_frame);
    else if (a.es == 1) hipLaunchKernelGGL((temporal_nr_kernel<uint8_t, false>), grid, block, 0, st, a, g.cells_per_row, g.blocks_per_frame);
    else if (a.vec) hipLaunchKernelGGL((temporal_nr_kernel<uint16_t, true>), grid, block, 0, st, a, g.cells_per_row, g.blocks_per_frame);
    else hipLaunchKernelGGL((temporal_nr_kernel<uint16_t, false>), grid, block, 0, st, a, g.cells_per_row, g.blocks_per_frame);
    return hipGetLastError();
}

} // namespace amt
