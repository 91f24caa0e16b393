// resize_surface_kernels.hip -- the resize of DESIGN.md section 6e (resize_kernels.hip) on decoder surfaces where they lie, source and
// destination in kind: NV12, interleaved LSB, P010 / P012 / P016 and planar MSB.  The result is defined on samples: de-interleave UV into
// U (even containers) and V (odd containers), take container >> s, apply the planar rule to every plane on its own, store every container
// as result << s.  No row is copied, so no low bit of the source survives, at equal sizes either.
// The shape is the planar kernels': work per wave, no barrier; horizontal first into the object's intermediate, which holds LSB samples,
// interleaved where the surfaces are.
// Horizontal: luma and planar chroma are dealt as in resize_h_kernel -- lanes are output columns.  An interleaved UV row is dealt in
// PAIRS: a wave's 64 lanes are up to 32 output columns times 2 components, lane = 2 * column + component, so the wave stores one
// contiguous run of the intermediate's UV row; a lane's tap j is container 2 * (start[col] + j) + comp of the staged span, which is
// 2 * es * (start[last] + K - start[first]) bytes (resize_pair_columns_per_wave, resize_region.h).  MSB: every staged dword is shifted
// once, packed, before the LDS write (the container-by-container path shifts per container), so the taps are read as samples.
// Vertical: layout-agnostic -- an interleaved frame is two planes, Y and UV of dst_w containers under the chroma program.  It is the
// planar cell with one packed left shift per stored dword where MSB.
// The rounding, the dealing of items, the vertical cell and the launchers' checks are resize_body.h's.  The two kernel bodies below
// repeat resize_kernels.hip's line for line where they can: one body called from both files' kernels changed the planar instructions.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"
#include "pack16.h"
#include "resize_body.h"

namespace amt {

// ---- horizontal ----
// the K taps of a lane, STEP containers apart in the staged span (2: one component of an interleaved row).  (resize_h_kernel keeps its
// loop written out: sharing this helper changed the planar instructions)
template <typename T, int KR, int STEP>
__device__ __forceinline__ int resize_taps(const T* taps, const int (&c)[KR > 0 ? KR : 1], const int* cf, int K)
{
    int acc = 0;
    if constexpr (KR > 0) {
#pragma unroll
        for (int j = 0; j < KR; ++j) acc = resize_mad(c[j], taps[j * STEP], acc);
    } else {
#pragma unroll 4
        for (int j = 0; j < K; ++j) acc = resize_mad(cf[j], taps[j * STEP], acc);
    }
    return acc;
}

// KR: as resize_h_kernel's.  MSB: containers are sample << shift.  IL: plane 1 is the one UV plane, dealt in pairs.
// (amdgpu_num_vgpr: left alone, the scheduler hoists every tap's LDS read of the 8-bit interleaved forms for 12 and 16 taps and ends at
// 67 and 69 registers; held to the budget of eight waves per SIMD it spills nothing: tests/test_isa_resize_surfaces.py)
template <typename T, int KR, bool MSB, bool IL>
__global__ __launch_bounds__(64 * kResizeWaves) __attribute__((amdgpu_num_vgpr(64)))
void resize_surface_h_kernel(ResizeStageArgs a, int runsY, int bandsY, int runsC, int bandsC, int shift)
{
    constexpr int ES = (int)sizeof(T), ESH = ES == 2 ? 1 : 0, NC = IL ? 1 : 2;
    static_assert(!MSB || ES == 2, "MSB-aligned containers are 16-bit");
    __shared__ __attribute__((aligned(16))) uint8_t lds[kResizeWaves][kResizeRegionBytes];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int itemsY = runsY * bandsY, itemsC = runsC * bandsC;
    const int item = blockIdx.x * kResizeWaves + wave;
    if (item >= itemsY + NC * itemsC) return;
    const ResizeItem it = resize_item(item, itemsY, itemsC);
    const bool chroma = it.plane != 0, pairs = IL && chroma;             // (wave-uniform)
    const int runs = chroma ? runsC : runsY;
    const int band = it.r / runs, run = it.r - band * runs;
    const ResizeProgramDev P = chroma ? a.prog[1] : a.prog[0];
    const ResizePlaneArgs pa = it.plane == 0 ? a.plane[0] : IL || it.plane == 1 ? a.plane[1] : a.plane[2];
    const int K = P.K, cpw = chroma ? a.cpw[1] : a.cpw[0], lines = chroma ? a.lines[1] : a.lines[0];
    const int col0 = run * cpw, ncols = min(cpw, P.D - col0);
    // a column's unit: one container, or the U and V containers of a pair (bytes 1 << ush); comp: which of the two the lane computes
    const int ush = pairs ? ESH + 1 : ESH, lcol = pairs ? lane >> 1 : lane, comp = pairs ? (lane & 1) << ESH : 0;
    const bool active = lcol < ncols;
    const int col = col0 + min(lcol, ncols - 1);                    // (a lane without a column computes its run's last one and stores nothing)
    const int span_lo = P.start[col0], span_hi = P.start[col0 + ncols - 1] + K;
    const int st = P.start[col];
    const int* cf = P.coeff + __mul24(col, K);
    int c[KR > 0 ? KR : 1];
    if constexpr (KR > 0) {
#pragma unroll
        for (int j = 0; j < KR; ++j) {
            const int v = cf[j < K ? j : 0];
            c[j] = j < K ? v : 0;
        }
    }
    // the region holds the row's bytes [A0, end): the span, from the 16 bytes it begins in where the loads are aligned ones
    const int A0 = a.vec ? (span_lo << ush) & ~15 : span_lo << ush, end = span_hi << ush, rowbytes = P.S << ush;
    uint8_t* region = lds[wave];
    const T* taps = reinterpret_cast<const T*>(region + ((st << ush) + comp - A0));
    const int row0 = band * kResizeRows, nrows = min(kResizeRows, lines - row0);
    const long long f = blockIdx.y;
    const uint8_t* srow = pa.src + f * pa.src_stride + (long long)row0 * pa.src_pitch;
    uint8_t* drow = pa.dst + f * pa.dst_stride + (long long)row0 * pa.dst_pitch + (long long)((col << ush) + comp);
#pragma unroll 1
    for (int r = 0; r < nrows; ++r, srow += pa.src_pitch, drow += pa.dst_pitch) {
        if (a.vec) {
#pragma unroll 1
            for (int b = A0 + 16 * lane; b < end; b += 16 * 64) {
                if (b + 16 <= rowbytes) {
                    uint4 q = *reinterpret_cast<const uint4*>(srow + b);
                    if constexpr (MSB) { q.x = pk_shr16(q.x, shift); q.y = pk_shr16(q.y, shift); q.z = pk_shr16(q.z, shift); q.w = pk_shr16(q.w, shift); }
                    *reinterpret_cast<uint4*>(region + (b - A0)) = q;
                } else {
#pragma unroll 1
                    for (int bb = b; bb < end; bb += ES) {
                        const T v = *reinterpret_cast<const T*>(srow + bb);
                        *reinterpret_cast<T*>(region + (bb - A0)) = MSB ? (T)(v >> shift) : v;
                    }
                }
            }
        } else {
#pragma unroll 1
            for (int b = A0 + ES * lane; b < end; b += ES * 64) {
                const T v = *reinterpret_cast<const T*>(srow + b);
                *reinterpret_cast<T*>(region + (b - A0)) = MSB ? (T)(v >> shift) : v;
            }
        }
        // the wave's own lanes wrote what its lanes now read: LDS serves a wave's accesses in order, the compiler must keep them so
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        int acc;
        if constexpr (IL) {
            acc = pairs ? resize_taps<T, KR, 2>(taps, c, cf, K) : resize_taps<T, KR, 1>(taps, c, cf, K);
        } else {
            acc = resize_taps<T, KR, 1>(taps, c, cf, K);
        }
        if (active) *reinterpret_cast<T*>(drow) = (T)resize_round(acc, a.maxv);           // (the intermediate holds LSB samples)
        // ... and the next row's staging must stay behind these reads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

hipError_t launch_resize_surfaces_h(hipStream_t st, const ResizeStageArgs& a, int interleaved, int shift, int nframes)
{
    if (nframes <= 0) return hipSuccess;
    if (!interleaved && !shift) return hipErrorInvalidValue;                             // planar LSB planes are launch_resize_h's
    ResizeGrid g;
    if (!resize_grid(a, true, interleaved ? 1 : 2, shift, nframes, g)) return hipErrorInvalidValue;
    const dim3 block(64 * kResizeWaves);
    const int K = a.prog[0].K > a.prog[1].K ? a.prog[0].K : a.prog[1].K;
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, g.grid, block, 0, st, a, g.per[0], g.across[0], g.per[1], g.across[1], shift); };
#define AMT_RESIZE_SURFACE_H(T, MSB, IL)                                  \
    do {                                                                  \
        if (K <= 8) go(resize_surface_h_kernel<T, 8, MSB, IL>);           \
        else if (K <= 12) go(resize_surface_h_kernel<T, 12, MSB, IL>);    \
        else if (K <= 16) go(resize_surface_h_kernel<T, 16, MSB, IL>);    \
        else go(resize_surface_h_kernel<T, 0, MSB, IL>);                  \
    } while (0)
    if (a.es == 1) AMT_RESIZE_SURFACE_H(uint8_t, false, true);
    else if (!shift) AMT_RESIZE_SURFACE_H(uint16_t, false, true);
    else if (interleaved) AMT_RESIZE_SURFACE_H(uint16_t, true, true);
    else AMT_RESIZE_SURFACE_H(uint16_t, true, false);
#undef AMT_RESIZE_SURFACE_H
    return hipGetLastError();
}

// ---- vertical ----
// VEC: resize_surface_vec16 (lane_rule.h).  chunks: waves per output row of the luma / chroma planes; nc: chroma planes (1: the UV plane)
template <typename T, bool VEC, bool MSB>
__global__ __launch_bounds__(64 * kResizeWaves)
void resize_surface_v_kernel(ResizeStageArgs a, int chunksY, int chunksC, int nc, int shift)
{
    constexpr int ES = (int)sizeof(T), PX = VEC ? 16 / ES : 1;
    static_assert(!MSB || ES == 2, "MSB-aligned containers are 16-bit");
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int itemsY = a.prog[0].D * chunksY, itemsC = a.prog[1].D * chunksC;
    const int item = blockIdx.x * kResizeWaves + wave;
    if (item >= itemsY + nc * itemsC) return;
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
        if (x0 + PX <= W) { resize_v_cell<T, PX, MSB>(src, pa.src_pitch, cf, K, a.maxv, dst, shift); return; }
#pragma unroll 1
        for (int x = x0; x < W; ++x, src += ES, dst += ES) resize_v_cell<T, 1, MSB>(src, pa.src_pitch, cf, K, a.maxv, dst, shift);
    } else {
        resize_v_cell<T, 1, MSB>(src, pa.src_pitch, cf, K, a.maxv, dst, shift);
    }
}

hipError_t launch_resize_surfaces_v(hipStream_t st, const ResizeStageArgs& a, int interleaved, int shift, int nframes)
{
    if (nframes <= 0) return hipSuccess;
    if (!interleaved && !shift) return hipErrorInvalidValue;                             // planar LSB planes are launch_resize_v's
    const int nc = interleaved ? 1 : 2;
    ResizeGrid g;
    if (!resize_grid(a, false, nc, shift, nframes, g)) return hipErrorInvalidValue;
    const dim3 block(64 * kResizeWaves);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, g.grid, block, 0, st, a, g.per[0], g.per[1], nc, shift); };
#define AMT_RESIZE_SURFACE_V(T, MSB)                                      \
    do {                                                                  \
        if (a.vec) go(resize_surface_v_kernel<T, true, MSB>);             \
        else go(resize_surface_v_kernel<T, false, MSB>);                  \
    } while (0)
    if (a.es == 1) AMT_RESIZE_SURFACE_V(uint8_t, false);
    else if (!shift) AMT_RESIZE_SURFACE_V(uint16_t, false);
    else AMT_RESIZE_SURFACE_V(uint16_t, true);
#undef AMT_RESIZE_SURFACE_V
    return hipGetLastError();
}

} // namespace amt
