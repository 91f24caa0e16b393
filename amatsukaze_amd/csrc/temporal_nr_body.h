// temporal_nr_body.h -- the cell of the temporal noise reduction, one text for temporal_nr_kernels.hip (planar LSB planes: MSB = false,
// IL = false, shift 0) and temporal_nr_surface_kernels.hip (decoder surfaces); device code only.  It is the reference's TemporalNRFilter
// (VideoFilter.hpp:156-211; the GUI's "temporal stabilisation", KTemporalNR(3, 1) in the server's chain), byte for byte.
// Per luma pixel (x, y) with its chroma sample (cx, cy) = (x >> 1, interlaced ? ((y >> 1) & ~1) | (y & 1) : y >> 1): a window frame
// passes where |dY| + |dU| + |dV| against the centre frame is at most thresh; the output is (T)(0.5f + sum over the passing frames, in
// window order, of fl(fl(1.f / count) * sample)) -- the product rounded, then the sum, no FMA (build.py compiles everything with
// -ffp-contract=off; tests/test_isa_temporal_nr.py and tests/test_isa_temporal_nr_surfaces.py look at the instructions).
// A chroma sample is filtered with the pass mask of ONE luma pixel: the even column of the first of the two luma rows that map to it.
// Shape: a lane owns the columns [x0, x0 + PX) of those two luma rows and the chroma under them; it walks the window twice, once for the
// counts and once for the sums, re-reading the samples (the second walk is served by the caches); 1.f / count comes from a table the
// compiler forms on the host.  Vector form: 16-byte luma accesses and, planar, an 8-byte run of each chroma row; interleaved, a lane's
// chroma is ONE 16-byte run of the UV row (8 pairs at 8 bits, 4 pairs at 16), de-interleaved in registers -- three 16-byte loads per
// window frame and three 16-byte stores per cell.  MSB forms shift each loaded dword once before any arithmetic and each stored dword
// once (packed 16-bit shifts).  The narrow form goes two luma columns per lane, container by container, one U and one V container
// beside each other where interleaved; the kernels send a row's last columns through it.  No LDS, no atomics, no scratch.
// (Measured and dropped: one v_sad_u16 on the dwords of a 16-bit UV pair for |dU| + |dV| -- a third fewer vector instructions in the
// window loops and no less time: DESIGN.md section 4.)
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"
#include "pack16.h"

namespace amt {

// fl(1.f / count), count = 1 .. 127 (temporal_distance <= 63), rounded by the host compiler's constant evaluation
// (internal linkage: each of the two kernel files carries its own 512 bytes)
struct TemporalNRRecip { float v[128]; };
constexpr TemporalNRRecip temporal_nr_recip()
{
    TemporalNRRecip t{};
    for (int i = 1; i < 128; ++i) t.v[i] = 1.f / (float)i;
    return t;
}
__device__ const TemporalNRRecip kTemporalNRRecip = temporal_nr_recip();

// N samples (container >> s where MSB) at p: one 16- or 8-byte access (VEC), or container by container
template <typename T, bool VEC, bool MSB, int N>
__device__ __forceinline__ void tnr_read(const uint8_t* p, unsigned (&o)[N], int s)
{
    if constexpr (VEC) {
        constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
        unsigned w[N / PER];
        if constexpr (N / PER == 4) {
            const uint4 q = *reinterpret_cast<const uint4*>(p);
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
            static_assert(N / PER == 2, "a vector lane moves 16 bytes, or 8 bytes of a planar chroma row");
            const uint2 q = *reinterpret_cast<const uint2*>(p);
            w[0] = q.x; w[1] = q.y;
        }
        if constexpr (MSB) {
#pragma unroll
            for (int i = 0; i < N / PER; ++i) w[i] = pk_shr16(w[i], s);
        }
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] = (w[j / PER] >> (BITS * (j % PER))) & ((1u << BITS) - 1);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] = MSB ? (unsigned)reinterpret_cast<const T*>(p)[j] >> s : (unsigned)reinterpret_cast<const T*>(p)[j];
    }
}

// (T)v[j] by truncation as containers (sample << s where MSB), stored the way tnr_read reads
template <typename T, bool VEC, bool MSB, int N>
__device__ __forceinline__ void tnr_write(uint8_t* p, const float (&v)[N], int s)
{
    if constexpr (VEC) {
        constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
        unsigned w[N / PER] = {};
#pragma unroll
        for (int j = 0; j < N; ++j) w[j / PER] |= (unsigned)(T)v[j] << (BITS * (j % PER));
        if constexpr (MSB) {
#pragma unroll
            for (int i = 0; i < N / PER; ++i) w[i] = pk_shl16(w[i], s);
        }
        if constexpr (N / PER == 4) *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
        else *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) reinterpret_cast<T*>(p)[j] = MSB ? (T)((unsigned)(T)v[j] << s) : (T)v[j];
    }
}

// luma columns [x0, x0 + PX) of rows y0 and y1 and the chroma pairs [x0 / 2, (x0 + PX) / 2) of row cy, of output frame `out` whose
// centre is the batch's frame `centre`.  IL: the pairs are the PX containers of the UV row at srcU / dstU that start at container x0
template <typename T, bool VEC, bool MSB, bool IL, int PX>
__device__ __forceinline__ void tnr_cell(const TemporalNRArgs& a, int s, int out, int centre, int y0, int y1, int cy, int x0)
{
    constexpr int PC = PX / 2;
    struct Samples { unsigned y[2][PX], u[PC], v[PC]; };
    const long long xY = (long long)x0 * (int)sizeof(T), xC = IL ? xY : (long long)(x0 >> 1) * (int)sizeof(T);
    const long long sY0 = (long long)y0 * a.src_pitchY + xY, sY1 = (long long)y1 * a.src_pitchY + xY, sC = (long long)cy * a.src_pitchUV + xC;
    auto load = [&](int f, Samples& r) {
        const long long oY = (long long)f * a.src_strideY, oC = (long long)f * a.src_strideUV;
        tnr_read<T, VEC, MSB>(a.srcY + oY + sY0, r.y[0], s);
        tnr_read<T, VEC, MSB>(a.srcY + oY + sY1, r.y[1], s);
        if constexpr (IL) {
            unsigned uv[PX];
            tnr_read<T, VEC, MSB>(a.srcU + oC + sC, uv, s);
#pragma unroll
            for (int k = 0; k < PC; ++k) { r.u[k] = uv[2 * k]; r.v[k] = uv[2 * k + 1]; }
        } else {
            tnr_read<T, VEC, MSB>(a.srcU + oC + sC, r.u, s);
            tnr_read<T, VEC, MSB>(a.srcV + oC + sC, r.v, s);
        }
    };
    auto window = [&](int i) { return min(max(centre + i - a.d, a.lo), a.hi); };
    const int n = 2 * a.d + 1;
    const unsigned thresh = (unsigned)a.thresh;

    Samples c;
    load(centre, c);
    int count[2][PX] = {};
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        Samples r;
        load(window(i), r);
#pragma unroll
        for (int k = 0; k < PC; ++k) {
            const unsigned dc = __usad(c.u[k], r.u[k], __usad(c.v[k], r.v[k], 0u));
#pragma unroll
            for (int row = 0; row < 2; ++row)
#pragma unroll
                for (int j = 2 * k; j < 2 * k + 2; ++j) count[row][j] += __usad(c.y[row][j], r.y[row][j], dc) <= thresh ? 1 : 0;
        }
    }

    float factor[2][PX], sumY[2][PX], sumU[PC], sumV[PC];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        factor[0][j] = kTemporalNRRecip.v[count[0][j]];
        factor[1][j] = kTemporalNRRecip.v[count[1][j]];
        sumY[0][j] = sumY[1][j] = 0.5f;
    }
#pragma unroll
    for (int k = 0; k < PC; ++k) sumU[k] = sumV[k] = 0.5f;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        Samples r;
        load(window(i), r);
#pragma unroll
        for (int k = 0; k < PC; ++k) {
            const unsigned dc = __usad(c.u[k], r.u[k], __usad(c.v[k], r.v[k], 0u));
#pragma unroll
            for (int row = 0; row < 2; ++row)
#pragma unroll
                for (int j = 2 * k; j < 2 * k + 2; ++j) {
                    // (a frame that does not pass adds +0.0f, which changes no bit of a sum that starts at 0.5f)
                    const float coef = __usad(c.y[row][j], r.y[row][j], dc) <= thresh ? factor[row][j] : 0.f;
                    sumY[row][j] += coef * (float)r.y[row][j];
                    if (row == 0 && j == 2 * k) {
                        sumU[k] += coef * (float)r.u[k];
                        sumV[k] += coef * (float)r.v[k];
                    }
                }
        }
    }

    const long long oY = (long long)out * a.dst_strideY + xY, oC = (long long)out * a.dst_strideUV + (long long)cy * a.dst_pitchUV + xC;
    tnr_write<T, VEC, MSB>(a.dstY + oY + (long long)y0 * a.dst_pitchY, sumY[0], s);
    tnr_write<T, VEC, MSB>(a.dstY + oY + (long long)y1 * a.dst_pitchY, sumY[1], s);
    if constexpr (IL) {
        float uv[PX];
#pragma unroll
        for (int k = 0; k < PC; ++k) { uv[2 * k] = sumU[k]; uv[2 * k + 1] = sumV[k]; }
        tnr_write<T, VEC, MSB>(a.dstU + oC, uv, s);
    } else {
        tnr_write<T, VEC, MSB>(a.dstU + oC, sumU, s);
        tnr_write<T, VEC, MSB>(a.dstV + oC, sumV, s);
    }
}

} // namespace amt
