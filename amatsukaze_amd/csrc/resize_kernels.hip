// resize_kernels.hip -- the resize of DESIGN.md section 6e ("parity unpinned": BlackmanResize is a built-in of the reference's AviSynth host,
// only the server's script text calls it, Misc.cs:1423) on planar LSB planes in HBM: integer, exact.  Two stages, always horizontal
// first; each is one launch for the luma and both chroma planes of every frame of a round.  Per output sample
//   clamp((sum_j coeff[i][j] * s[start[i] + j] + 8192) >> 14, 0, maxv)
// in int32 (the host has checked that no sum leaves it: resize_plan.hpp).  Every coefficient and sample is far inside 24 bits, so the
// multiply-adds are the 24-bit, full-rate ones; tests/test_isa_resize.py looks at the instructions.
//
// Work is dealt out per WAVE: a workgroup is kResizeWaves waves that never meet (no barrier).
// Horizontal: a wave owns a run of up to 64 output columns of kResizeRows rows.  Lanes are output columns; a lane keeps its start and its
// K coefficients in registers (forms for K up to 8, 12 and 16, padded with zero taps; above that the lane walks the table).  Per row the
// wave stages the source span its columns read -- start[last] + K - start[first] samples, 101 at 3:2 -- into an LDS region of its own,
// with aligned 16-byte loads where resize_vec16 holds (the span's bytes behind the row's last whole 16 go container by container), then
// each lane reads its taps from LDS.
// Vertical: a wave owns 64 lanes' worth of one output row, so the row's start and coefficients are wave-uniform and come through the
// scalar unit; a lane owns 16 bytes of the row and walks the K intermediate rows under it with 16-byte loads (a row's last containers,
// and everything where resize_vec16 does not hold, go container by container).  No LDS.
// Frame offsets are 64-bit.  What the decoder-surface kernels share with these is in resize_body.h.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"
#include "resize_body.h"

namespace amt {

// ---- horizontal ----
// KR: taps a lane keeps in registers (K <= KR, the rest zero); 0: the lane reads its coefficients from the table, tap by tap
template <typename T, int KR>
__global__ __launch_bounds__(64 * kResizeWaves)
void resize_h_kernel(ResizeStageArgs a, int runsY, int bandsY, int runsC, int bandsC)
{
    constexpr int ES = (int)sizeof(T);
    __shared__ __attribute__((aligned(16))) uint8_t lds[kResizeWaves][kResizeRegionBytes];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int itemsY = runsY * bandsY, itemsC = runsC * bandsC;
    const int item = blockIdx.x * kResizeWaves + wave;
    if (item >= itemsY + 2 * itemsC) return;
    const ResizeItem it = resize_item(item, itemsY, itemsC);
    // (the arguments are picked with selects, not indexed: an index would be vector address arithmetic with a full-width multiply)
    const bool chroma = it.plane != 0;
    const int runs = chroma ? runsC : runsY;
    const int band = it.r / runs, run = it.r - band * runs;
    const ResizeProgramDev P = chroma ? a.prog[1] : a.prog[0];
    const ResizePlaneArgs pa = it.plane == 0 ? a.plane[0] : it.plane == 1 ? a.plane[1] : a.plane[2];
    const int K = P.K, cpw = chroma ? a.cpw[1] : a.cpw[0], lines = chroma ? a.lines[1] : a.lines[0];
    const int col0 = run * cpw, ncols = min(cpw, P.D - col0);
    const bool active = lane < ncols;
    const int col = col0 + min(lane, ncols - 1);                    // (a lane without a column computes its run's last one and stores nothing)
    const int span_lo = P.start[col0], span_hi = P.start[col0 + ncols - 1] + K;
    const int st = P.start[col];
    const int* cf = P.coeff + __mul24(col, K);
    int c[KR > 0 ? KR : 1];
    if constexpr (KR > 0) {
#pragma unroll
        for (int j = 0; j < KR; ++j) {
            const int v = cf[j < K ? j : 0];                            // (every load issued before the first wait: a select, not a branch)
            c[j] = j < K ? v : 0;
        }
    }
    // the region holds the row's bytes [A0, end): the span, from the 16 bytes it begins in where the loads are aligned ones
    const int A0 = a.vec ? (span_lo * ES) & ~15 : span_lo * ES, end = span_hi * ES, rowbytes = P.S * ES;
    uint8_t* region = lds[wave];
    const T* taps = reinterpret_cast<const T*>(region) + (st - A0 / ES);
    const int row0 = band * kResizeRows, nrows = min(kResizeRows, lines - row0);
    const long long f = blockIdx.y;
    const uint8_t* srow = pa.src + f * pa.src_stride + (long long)row0 * pa.src_pitch;
    uint8_t* drow = pa.dst + f * pa.dst_stride + (long long)row0 * pa.dst_pitch + (long long)col * ES;
#pragma unroll 1
    for (int r = 0; r < nrows; ++r, srow += pa.src_pitch, drow += pa.dst_pitch) {
        if (a.vec) {
#pragma unroll 1
            for (int b = A0 + 16 * lane; b < end; b += 16 * 64) {
                if (b + 16 <= rowbytes) {
                    *reinterpret_cast<uint4*>(region + (b - A0)) = *reinterpret_cast<const uint4*>(srow + b);
                } else {
#pragma unroll 1
                    for (int bb = b; bb < end; bb += ES) *reinterpret_cast<T*>(region + (bb - A0)) = *reinterpret_cast<const T*>(srow + bb);
                }
            }
        } else {
#pragma unroll 1
            for (int b = A0 + ES * lane; b < end; b += ES * 64) *reinterpret_cast<T*>(region + (b - A0)) = *reinterpret_cast<const T*>(srow + b);
        }
        // the wave's own lanes wrote what its lanes now read: LDS serves a wave's accesses in order, the compiler must keep them so
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // (the tap loop stays written out: through resize_surface_kernels.hip's resize_taps it compiled to other instructions)
        int acc = 0;
        if constexpr (KR > 0) {
#pragma unroll
            for (int j = 0; j < KR; ++j) acc = resize_mad(c[j], taps[j], acc);
        } else {
#pragma unroll 4
            for (int j = 0; j < K; ++j) acc = resize_mad(cf[j], taps[j], acc);
        }
        if (active) *reinterpret_cast<T*>(drow) = (T)resize_round(acc, a.maxv);
        // ... and the next row's staging must stay behind these reads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

hipError_t launch_resize_h(hipStream_t st, const ResizeStageArgs& a, int nframes)
{
    if (nframes <= 0) return hipSuccess;
    ResizeGrid g;
    if (!resize_grid(a, true, 2, 0, nframes, g)) return hipErrorInvalidValue;
    const dim3 block(64 * kResizeWaves);
    const int K = a.prog[0].K > a.prog[1].K ? a.prog[0].K : a.prog[1].K;
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, g.grid, block, 0, st, a, g.per[0], g.across[0], g.per[1], g.across[1]); };
    with_sample_type(a.es == 1 ? 8 : 16, [&](auto pix) {
        using T = decltype(pix);
        if (K <= 8) go(resize_h_kernel<T, 8>);
        else if (K <= 12) go(resize_h_kernel<T, 12>);
        else if (K <= 16) go(resize_h_kernel<T, 16>);
        else go(resize_h_kernel<T, 0>);
    });
    return hipGetLastError();
}

// ---- vertical ----
// VEC: resize_vec16 (lane_rule.h).  chunks: waves per output row of the luma / chroma planes
template <typename T, bool VEC>
__global__ __launch_bounds__(64 * kResizeWaves)
void resize_v_kernel(ResizeStageArgs a, int chunksY, int chunksC)
{
    constexpr int ES = (int)sizeof(T), PX = VEC ? 16 / ES : 1;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int itemsY = a.prog[0].D * chunksY, itemsC = a.prog[1].D * chunksC;
    const int item = blockIdx.x * kResizeWaves + wave;
    if (item >= itemsY + 2 * itemsC) return;
    const ResizeItem it = resize_item(item, itemsY, itemsC);
    const bool chroma = it.plane != 0;
    const int chunks = chroma ? chunksC : chunksY;
    const int y = it.r / chunks, chunk = it.r - y * chunks;
    const ResizeProgramDev P = chroma ? a.prog[1] : a.prog[0];
    const ResizePlaneArgs pa = it.plane == 0 ? a.plane[0] : it.plane == 1 ? a.plane[1] : a.plane[2];
    const int W = chroma ? a.lines[1] : a.lines[0], x0 = (chunk * 64 + lane) * PX;
    if (x0 >= W) return;
    const int K = P.K;
    const int* cf = P.coeff + y * K;
    const long long f = blockIdx.y;
    const uint8_t* src = pa.src + f * pa.src_stride + (long long)P.start[y] * pa.src_pitch + (long long)x0 * ES;
    uint8_t* dst = pa.dst + f * pa.dst_stride + (long long)y * pa.dst_pitch + (long long)x0 * ES;
    if constexpr (VEC) {
        if (x0 + PX <= W) { resize_v_cell<T, PX, false>(src, pa.src_pitch, cf, K, a.maxv, dst, 0); return; }
#pragma unroll 1
        for (int x = x0; x < W; ++x, src += ES, dst += ES) resize_v_cell<T, 1, false>(src, pa.src_pitch, cf, K, a.maxv, dst, 0);
    } else {
        resize_v_cell<T, 1, false>(src, pa.src_pitch, cf, K, a.maxv, dst, 0);
    }
}

hipError_t launch_resize_v(hipStream_t st, const ResizeStageArgs& a, int nframes)
{
    if (nframes <= 0) return hipSuccess;
    ResizeGrid g;
    if (!resize_grid(a, false, 2, 0, nframes, g)) return hipErrorInvalidValue;
    const dim3 block(64 * kResizeWaves);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, g.grid, block, 0, st, a, g.per[0], g.per[1]); };
    with_sample_type(a.es == 1 ? 8 : 16, [&](auto pix) {
        using T = decltype(pix);
        if (a.vec) go(resize_v_kernel<T, true>);
        else go(resize_v_kernel<T, false>);
    });
    return hipGetLastError();
}

} // namespace amt
