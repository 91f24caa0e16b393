// stats_kernels.hip -- whole-frame field-difference / combing metrics (self-specified).
//
// Streaming reduction over the Y plane: every byte of every frame is read from HBM once.  A thread owns a 16-byte-wide column of a
// tile of 24 rows (8-bit samples; 16 rows at 16 bits) for a RUN of consecutive frames ((tile, column) pairs are dealt densely to the threads of the grid), so the vertical
// neighbours (rows y-1, y+1) and the previous frame's rows are all in the thread's own registers -- no LDS staging, no re-reads
// except the two halo rows per tile.  Loads are 16 B per lane, 64 lanes = 1 KiB contiguous per row.  The per-byte work is done four
// pixels at a time with v_sad_u8 / v_lerp_u8 (two per instruction for 16-bit samples).
//
// What bounds it (profiles/r04_notes.md): with the whole device the kernel moves 6.1 TB/s of actual traffic (1.15x its algorithmic
// bytes: 128-byte lines against a 1472-byte pitch, halo rows, the frame before a run) -- HBM.  Given a PART of the device
// (hipExtStreamCreateWithCUMask, to run beside the VALU-bound logo kernels) its rate scales with the CUs it owns: per CU it is bound
// by the vector ALU and by the bytes a CU keeps in flight.  Hence the form below: raw buffer loads (one VGPR of address for the whole
// tile, rows outside the frame come back as zeros from the bounds check -- no 64-bit address arithmetic, no selects), the even-row
// vertical detail of the previous frame carried over instead of recomputed, wave sums on DPP instead of LDS permutes.
//
// Per frame n (prev = frame n-1; rows 1..H-2 for the vertical metrics), all sums of absolute values:
//   0 DIFF_TOP   sum_{y even} |Y_n[y] - Y_prev[y]|          3 COMB       sum |Y_n[y] - avg(Y_n[y-1], Y_n[y+1])|
//   1 DIFF_BOT   sum_{y odd}  |Y_n[y] - Y_prev[y]|          4 COMB_PREV  same on the weave (even rows of n, odd rows of prev)
//   2 VERT_SAME  sum |Y_n[y-1] - Y_n[y+1]|                  5 SUM        sum Y_n
//   6 VERT_PREV  VERT_SAME of that weave                    7 reserved (0)
// avg(a,c) = (a + c) >> 1 per sample.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"
#include "stats_body.h"

namespace amt {

hipError_t launch_frame_stats(hipStream_t st, int bits, const FrameBatch& b, int W, int H, const void* dprevY, int nframes, unsigned long long* dout)
{
    if (nframes <= 0) return hipSuccess;
    if (b.shift) return launch_frame_stats_msb(st, bits, b, W, H, dprevY, nframes, dout);
    const int es = bits <= 8 ? 1 : 2;
    if (b.es != es) return hipErrorInvalidValue;
    const StatGrid g = stat_grid(es, b.pitchY, W, H, nframes);
    if (!g.fits) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(dout, 0, (size_t)nframes * kStatWords * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    dim3 grid((unsigned)g.gx, (unsigned)g.gy), block(kStatThreads);
#define AMT_STATS_LAUNCH(E, RG, BF)                                                                                                          \
    hipLaunchKernelGGL((frame_stats_kernel<E, RG, BF, false>), grid, block, 0, st, (const uint8_t*)b.Y, b.strideY, b.pitchY * es, g.row_bytes, H, \
                       (const uint8_t*)dprevY, nframes, g.col_groups, dout, 0)
    if (es == 1) { if (!g.buf) AMT_STATS_LAUNCH(1, true, false); else if (g.ragged) AMT_STATS_LAUNCH(1, true, true); else AMT_STATS_LAUNCH(1, false, true); }
    else { if (!g.buf) AMT_STATS_LAUNCH(2, true, false); else if (g.ragged) AMT_STATS_LAUNCH(2, true, true); else AMT_STATS_LAUNCH(2, false, true); }
#undef AMT_STATS_LAUNCH
    return hipGetLastError();
}

} // namespace amt
