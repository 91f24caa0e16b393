// deband_body.h -- the text that deband_kernels.hip (planar LSB planes) and deband_surface_kernels.hip (decoder surfaces in kind) share:
// the cell that filters a lane's 16 bytes of an output row out of LDS, the load of its table entries, the row offsets from 24-bit
// products, and the number of loads a staging lane keeps in flight.  (The staging itself stands in either file: as a function shared by
// both it changed the planar kernels' register allocation.)  LDS always holds SAMPLES: an MSB form shifts while it stages, so the cell is
// the LSB cell whatever the containers were.  STEP is the distance in containers between horizontal neighbours of one component: 1 in a
// plane of its own, 2 in an interleaved UV row, where a reference of a U container is the U container 2 * dx further on.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"

namespace amt {

// rows * pitch for a handful of rows (below 2^8) and a pitch below 2^31, from two 24-bit products
__device__ __forceinline__ long long deband_rows(int rows, int pitch)
{
    return (long long)__umul24(rows, pitch & 0xFFFFFF) + ((long long)__umul24(rows, (unsigned)pitch >> 24) << 24);
}

// The 16 / es pixels of a lane: centre points at the first one in LDS, dxw / dyw hold their table entries, one byte each.  NS: the
// references of a pixel (1, 2, 4: sample 0, 1, 2); BF: blur_first
template <typename T, int NS, bool BF, int STEP = 1>
__device__ __forceinline__ void deband_cell(const uint8_t* centre, const unsigned* dxw, const unsigned* dyw, unsigned thresh, unsigned (&out)[4])
{
    constexpr int ES = (int)sizeof(T), PX = 16 / ES, PER = 4 / ES, BITS = 8 * ES, ROW = deband_lds_pitch(ES) / ES;
    static_assert(ROW % STEP == 0, "the LDS row is a whole number of steps");
    const uint4 q = *reinterpret_cast<const uint4*>(centre);
    const unsigned cw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = 0;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const unsigned c = (cw[j / PER] >> (BITS * (j % PER))) & ((1u << BITS) - 1);
        const int dx = (int)(int8_t)(dxw[j / 4] >> (8 * (j % 4))), dy = (int)(int8_t)(dyw[j / 4] >> (8 * (j % 4)));
        const T* pc = reinterpret_cast<const T*>(centre) + j;
        const int o0 = STEP * (__mul24(dy, ROW / STEP) + dx);           // dy * ROW + STEP * dx: the step rides in the address's shift
        const unsigned p0 = pc[o0];
        unsigned avg = p0, far = __usad(p0, c, 0u);
        if constexpr (NS >= 2) {
            const unsigned p1 = pc[-o0];
            avg += p1;
            far = max(far, __usad(p1, c, 0u));
        }
        if constexpr (NS == 4) {
            const int o2 = STEP * (__mul24(dx, ROW / STEP) - dy);
            const unsigned p2 = pc[o2], p3 = pc[-o2];
            avg += p2 + p3;
            far = max(far, max(__usad(p2, c, 0u), __usad(p3, c, 0u)));
        }
        if constexpr (NS == 2) avg = (avg + 1) >> 1;
        if constexpr (NS == 4) avg = (avg + 2) >> 2;
        const unsigned v = (BF || NS == 1 ? __usad(avg, c, 0u) : far) <= thresh ? avg : c;
        out[j / PER] |= v << (BITS * (j % PER));
    }
}

// the table entries of a lane's 16 / es pixels: one vector load of dx and one of dy (the rows are padded to 16 entries)
template <int PX> struct DebandOffsets { unsigned dx[PX / 4], dy[PX / 4]; };
template <int PX>
__device__ __forceinline__ DebandOffsets<PX> deband_offsets(const int8_t* tdx, const int8_t* tdy)
{
    DebandOffsets<PX> o;
    if constexpr (PX == 16) {
        const uint4 u = *reinterpret_cast<const uint4*>(tdx), v = *reinterpret_cast<const uint4*>(tdy);
        o.dx[0] = u.x; o.dx[1] = u.y; o.dx[2] = u.z; o.dx[3] = u.w;
        o.dy[0] = v.x; o.dy[1] = v.y; o.dy[2] = v.z; o.dy[3] = v.w;
    } else {
        const uint2 u = *reinterpret_cast<const uint2*>(tdx), v = *reinterpret_cast<const uint2*>(tdy);
        o.dx[0] = u.x; o.dx[1] = u.y;
        o.dy[0] = v.x; o.dy[1] = v.y;
    }
    return o;
}

constexpr int kStageBatch = 10;                                        // 16-byte loads a lane has in flight while it stages

} // namespace amt
