// resize_body.h -- what resize_kernels.hip (planar LSB planes: MSB = false, shift 0) and resize_surface_kernels.hip (decoder surfaces)
// have in one text: the multiply-add and the rounding of DESIGN.md section 6e, how a frame's items are dealt to planes, the vertical
// stage's cell with its load and store, and on the host the launchers' argument check and grids.  The bodies of the four __global__
// functions and the horizontal tap loops are not here: moved into shared functions they compiled to other instructions.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"
#include "pack16.h"

namespace amt {

__device__ __forceinline__ int resize_mad(int c, unsigned s, int acc) { return __mul24(c, (int)s) + acc; }
__device__ __forceinline__ int resize_round(int acc, int maxv) { return min(max((acc + 8192) >> 14, 0), maxv); }

// which plane, and which of its items, the item `r` of a frame is: luma items first, then U's (or UV's), then V's
struct ResizeItem { int plane, r; };
__device__ __forceinline__ ResizeItem resize_item(int r, int itemsY, int itemsC)
{
    // (wave-uniform, and said so: the plane number indexes the kernel's arguments, which is then scalar address arithmetic)
    const int plane = r < itemsY ? 0 : r < itemsY + itemsC ? 1 : 2;
    return ResizeItem{__builtin_amdgcn_readfirstlane(plane), __builtin_amdgcn_readfirstlane(r - (plane == 0 ? 0 : plane == 1 ? itemsY : itemsY + itemsC))};
}

// ---- vertical ----
// N containers of LSB samples at p as integers: one 16-byte access or one container
template <typename T, int N>
__device__ __forceinline__ void resize_load(const uint8_t* p, unsigned (&o)[N])
{
    if constexpr (N == 1) {
        o[0] = *reinterpret_cast<const T*>(p);
    } else {
        static_assert(N * sizeof(T) == 16, "a vector lane moves 16 bytes");
        constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] = (w[j / PER] >> (BITS * (j % PER))) & ((1u << BITS) - 1);
    }
}

// ... and N results as containers, result << shift where MSB: one packed shift per stored dword
template <typename T, int N, bool MSB>
__device__ __forceinline__ void resize_store(uint8_t* p, const int (&acc)[N], int maxv, int shift)
{
    if constexpr (N == 1) {
        const int v = resize_round(acc[0], maxv);
        *reinterpret_cast<T*>(p) = MSB ? (T)(v << shift) : (T)v;
    } else {
        constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
        unsigned w[4] = {};
#pragma unroll
        for (int j = 0; j < N; ++j) w[j / PER] |= (unsigned)resize_round(acc[j], maxv) << (BITS * (j % PER));
        if constexpr (MSB) {
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = pk_shl16(w[i], shift);
        }
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// N containers of an output row from the K rows at src, src_pitch apart; cf: the row's coefficients (wave-uniform)
template <typename T, int N, bool MSB>
__device__ __forceinline__ void resize_v_cell(const uint8_t* src, int src_pitch, const int* cf, int K, int maxv, uint8_t* dst, int shift)
{
    int acc[N] = {};
#pragma unroll 4
    for (int j = 0; j < K; ++j, src += src_pitch) {
        const int c = cf[j];
        unsigned s[N];
        resize_load<T, N>(src, s);
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = resize_mad(c, s[n], acc[n]);
    }
    resize_store<T, N, MSB>(dst, acc, maxv, shift);
}

// ---- host: what the four launchers check and how they deal a frame out ----
// nc: the chroma planes of a frame -- 2, or 1 where U and V are one interleaved plane (plane[2] is then not looked at)
inline bool resize_args_ok(const ResizeStageArgs& a, int nc, int shift, int nframes)
{
    if ((a.es != 1 && a.es != 2) || a.maxv < 255 || a.maxv > 65535 || nframes > 65535) return false;
    if (shift < 0 || shift > 7 || (shift && a.es != 2)) return false;
    for (int k = 0; k < 2; ++k)
        if (!a.prog[k].start || !a.prog[k].coeff || a.prog[k].S <= 0 || a.prog[k].D <= 0 || a.prog[k].K <= 0 || a.prog[k].K > a.prog[k].S || a.lines[k] <= 0 ||
            a.prog[k].S >= (1 << 23) || a.prog[k].D >= (1 << 23))
            return false;
    for (int p = 0; p < 1 + nc; ++p)
        if (!a.plane[p].src || !a.plane[p].dst || a.plane[p].src_pitch <= 0 || a.plane[p].dst_pitch <= 0) return false;
    return true;
}

// A stage's grid: a frame is per[0] * across[0] luma items and nc times per[1] * across[1] chroma items, one wave each, kResizeWaves to
// a block; frames are the grid's y.  Horizontal: per = runs of cpw columns, across = bands of kResizeRows rows (a run of an
// interleaved plane is at most 32 pairs); vertical: per = chunks of 64 lanes in an output row, across = the rows (prog[].D)
struct ResizeGrid { int per[2], across[2]; dim3 grid; };
inline bool resize_grid(const ResizeStageArgs& a, bool horizontal, int nc, int shift, int nframes, ResizeGrid& g)
{
    if (!resize_args_ok(a, nc, shift, nframes)) return false;
    long long items = 0;
    for (int k = 0; k < 2; ++k) {
        if (horizontal) {
            if (a.cpw[k] < 1 || a.cpw[k] > (k && nc == 1 ? 32 : 64)) return false;
            g.per[k] = (a.prog[k].D + a.cpw[k] - 1) / a.cpw[k];
            g.across[k] = (a.lines[k] + kResizeRows - 1) / kResizeRows;
        } else {
            const int px = a.vec ? 16 / a.es : 1;
            g.per[k] = ((a.lines[k] + px - 1) / px + 63) / 64;
            g.across[k] = a.prog[k].D;
        }
        items += (k ? nc : 1) * (long long)g.per[k] * g.across[k];
    }
    if (items > 0x7FFFFF00LL) return false;
    g.grid = dim3((unsigned)((items + kResizeWaves - 1) / kResizeWaves), (unsigned)nframes);
    return true;
}

} // namespace amt
