// temporal_nr_surface_kernels.hip -- the temporal noise reduction (temporal_nr_kernels.hip) on decoder surfaces
// where they lie, source and destination in kind: NV12, interleaved LSB, P010 / P012 and planar MSB.  The result is defined on samples:
// de-interleave UV into U (even containers) and V (odd containers), take container >> s, apply the planar rule, store every container
// as result << s with zero low bits, re-interleave.  Nothing is copied from the source, so low bits never survive.
// The shape is the planar kernel's: a lane owns the columns [x0, x0 + PX) of the two luma rows that share a chroma row and the chroma
// under them; it walks the window twice, once for the counts and once for the sums in window order, 1.f / count from a table the
// compiler forms on the host, the product rounded, then the sum, no FMA.  Vector form: 16-byte luma accesses; interleaved, a lane's
// chroma is ONE 16-byte run of the UV row (8 pairs at 8 bits, 4 pairs at 16), de-interleaved in registers -- three 16-byte loads per
// window frame and three 16-byte stores per cell; planar MSB keeps the planar kernel's two 8-byte chroma runs.  MSB forms shift each
// loaded dword once before any arithmetic and each stored dword once (packed 16-bit shifts).  (Measured and dropped: one v_sad_u16 on
// the dwords of a 16-bit UV pair for |dU| + |dV| -- a third fewer vector instructions in the window loops and no less time: DESIGN.md
// section 4.)  The row's last columns go two luma columns at a time; the narrow form goes two luma columns per lane, container by
// container, one U and one V container beside each other.  No LDS, no atomics, no scratch; one launch.  The cell below repeats temporal_nr_kernels.hip's, as render_surface_kernels.hip
// repeats kfm_render_kernel's and for the same reason: the planar kernels are to stay exactly as they were.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"
#include "pack16.h"

namespace amt {

// fl(1.f / count), count = 1 .. 127 (temporal_distance <= 63), rounded by the host compiler's constant evaluation
struct TemporalNRSurfaceRecip { float v[128]; };
constexpr TemporalNRSurfaceRecip temporal_nr_surface_recip()
{
    TemporalNRSurfaceRecip t{};
    for (int i = 1; i < 128; ++i) t.v[i] = 1.f / (float)i;
    return t;
}
__device__ const TemporalNRSurfaceRecip kTemporalNRSurfaceRecip = temporal_nr_surface_recip();

// N samples (container >> s where MSB) at p: one 16- or 8-byte access (VEC), or container by container
template <typename T, bool VEC, bool MSB, int N>
__device__ __forceinline__ void tnrs_read(const uint8_t* p, unsigned (&o)[N], int s)
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

// (T)v[j] by truncation as containers (sample << s where MSB), stored the way tnrs_read reads
template <typename T, bool VEC, bool MSB, int N>
__device__ __forceinline__ void tnrs_write(uint8_t* p, const float (&v)[N], int s)
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
__device__ __forceinline__ void tnrs_cell(const TemporalNRArgs& a, int s, int out, int centre, int y0, int y1, int cy, int x0)
{
    constexpr int PC = PX / 2;
    struct Samples { unsigned y[2][PX], u[PC], v[PC]; };
    const long long xY = (long long)x0 * (int)sizeof(T), xC = IL ? xY : (long long)(x0 >> 1) * (int)sizeof(T);
    const long long sY0 = (long long)y0 * a.src_pitchY + xY, sY1 = (long long)y1 * a.src_pitchY + xY, sC = (long long)cy * a.src_pitchUV + xC;
    auto load = [&](int f, Samples& r) {
        const long long oY = (long long)f * a.src_strideY, oC = (long long)f * a.src_strideUV;
        tnrs_read<T, VEC, MSB>(a.srcY + oY + sY0, r.y[0], s);
        tnrs_read<T, VEC, MSB>(a.srcY + oY + sY1, r.y[1], s);
        if constexpr (IL) {
            unsigned uv[PX];
            tnrs_read<T, VEC, MSB>(a.srcU + oC + sC, uv, s);
#pragma unroll
            for (int k = 0; k < PC; ++k) { r.u[k] = uv[2 * k]; r.v[k] = uv[2 * k + 1]; }
        } else {
            tnrs_read<T, VEC, MSB>(a.srcU + oC + sC, r.u, s);
            tnrs_read<T, VEC, MSB>(a.srcV + oC + sC, r.v, s);
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
        factor[0][j] = kTemporalNRSurfaceRecip.v[count[0][j]];
        factor[1][j] = kTemporalNRSurfaceRecip.v[count[1][j]];
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
    tnrs_write<T, VEC, MSB>(a.dstY + oY + (long long)y0 * a.dst_pitchY, sumY[0], s);
    tnrs_write<T, VEC, MSB>(a.dstY + oY + (long long)y1 * a.dst_pitchY, sumY[1], s);
    if constexpr (IL) {
        float uv[PX];
#pragma unroll
        for (int k = 0; k < PC; ++k) { uv[2 * k] = sumU[k]; uv[2 * k + 1] = sumV[k]; }
        tnrs_write<T, VEC, MSB>(a.dstU + oC, uv, s);
    } else {
        tnrs_write<T, VEC, MSB>(a.dstU + oC, sumU, s);
        tnrs_write<T, VEC, MSB>(a.dstV + oC, sumV, s);
    }
}

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
        if (x0 + PX <= a.W) { tnrs_cell<T, true, MSB, IL, PX>(a, s, out, centre, y0, y1, cy, x0); return; }
#pragma unroll 1
        for (int x = x0; x < a.W; x += 2) tnrs_cell<T, false, MSB, IL, 2>(a, s, out, centre, y0, y1, cy, x);
    } else {
        tnrs_cell<T, false, MSB, IL, 2>(a, s, out, centre, y0, y1, cy, x0);
    }
}

hipError_t launch_temporal_nr_surfaces(hipStream_t st, const TemporalNRArgs& a, int interleaved, int shift, int nout)
{
    if (nout <= 0) return hipSuccess;
    if ((a.es != 1 && a.es != 2) || a.d < 0 || a.d > 63 || a.W <= 0 || a.H <= 0 || (a.W & 1) || (a.H & 1)) return hipErrorInvalidValue;
    if (shift < 0 || shift > 7 || (shift && a.es != 2)) return hipErrorInvalidValue;
    if (!interleaved && !shift) return hipErrorInvalidValue;                             // planar LSB planes are launch_temporal_nr's
    const int px = a.vec ? 16 / a.es : 2;
    const long long cells_per_row = (a.W + px - 1) / px, cells = cells_per_row * (a.H >> 1);
    const long long blocks_per_frame = (cells + 255) / 256;
    if (cells > 0x7FFFFF00LL || blocks_per_frame * nout > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    dim3 grid((unsigned)(blocks_per_frame * nout)), block(256);
#define AMT_TNRS_LAUNCH(T, VEC, MSB, IL) \
    hipLaunchKernelGGL((temporal_nr_surfaces_kernel<T, VEC, MSB, IL>), grid, block, 0, st, a, (int)cells_per_row, (int)blocks_per_frame, shift)
    if (!interleaved) { if (a.vec) AMT_TNRS_LAUNCH(uint16_t, true, true, false); else AMT_TNRS_LAUNCH(uint16_t, false, true, false); }
    else if (shift) { if (a.vec) AMT_TNRS_LAUNCH(uint16_t, true, true, true); else AMT_TNRS_LAUNCH(uint16_t, false, true, true); }
    else if (a.es == 1) { if (a.vec) AMT_TNRS_LAUNCH(uint8_t, true, false, true); else AMT_TNRS_LAUNCH(uint8_t, false, false, true); }
    else { if (a.vec) AMT_TNRS_LAUNCH(uint16_t, true, false, true); else AMT_TNRS_LAUNCH(uint16_t, false, false, true); }
#undef AMT_TNRS_LAUNCH
    return hipGetLastError();
}

} // namespace amt
