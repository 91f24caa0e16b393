// temporal_nr_kernels.hip -- the reference's TemporalNRFilter (VideoFilter.hpp:156-211; the GUI's "temporal stabilisation", KTemporalNR(3, 1)
// in the server's chain) on planar LSB planes in HBM, byte for byte.  Per luma pixel (x, y) with its chroma sample (cx, cy) = (x >> 1,
// interlaced ? ((y >> 1) & ~1) | (y & 1) : y >> 1): a window frame passes where |dY| + |dU| + |dV| against the centre frame is at most
// thresh; the output is (T)(0.5f + sum over the passing frames, in window order, of fl(fl(1.f / count) * sample)) -- the product rounded,
// then the sum, no FMA (build.py compiles everything with -ffp-contract=off; tests/test_isa_temporal_nr.py looks at the instructions).
// A chroma sample is filtered with the pass mask of ONE luma pixel: the even column of the first of the two luma rows that map to it.
// Shape: a lane owns the columns [x0, x0 + PX) of those two luma rows and the chroma run under them; it walks the window twice, once for
// the counts and once for the sums, re-reading the samples (the second pass is served by the caches); 1.f / count comes from a table the
// compiler forms on the host.  Vector form: 16-byte luma and 8-byte chroma accesses, the row's last columns two at a time; the other form
// goes two luma columns per lane, container by container.  No LDS, no atomics, no scratch; one launch.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.hpp"

namespace amt {

// fl(1.f / count), count = 1 .. 127 (temporal_distance <= 63), rounded by the host compiler's constant evaluation
struct TemporalNRRecip { float v[128]; };
constexpr TemporalNRRecip temporal_nr_recip()
{
    TemporalNRRecip t{};
    for (int i = 1; i < 128; ++i) t.v[i] = 1.f / (float)i;
    return t;
}
__device__ const TemporalNRRecip kTemporalNRRecip = temporal_nr_recip();

// N containers at p as integers: one 16- or 8-byte access (VEC), or container by container
template <typename T, bool VEC, int N>
__device__ __forceinline__ void tnr_load(const uint8_t* p, unsigned (&o)[N])
{
    if constexpr (VEC) {
        constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
        unsigned w[N / PER];
        if constexpr (N / PER == 4) {
            const uint4 q = *reinterpret_cast<const uint4*>(p);
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
            static_assert(N / PER == 2, "a vector lane moves 16 luma bytes and 8 chroma bytes");
            const uint2 q = *reinterpret_cast<const uint2*>(p);
            w[0] = q.x; w[1] = q.y;
        }
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] = (w[j / PER] >> (BITS * (j % PER))) & ((1u << BITS) - 1);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] = reinterpret_cast<const T*>(p)[j];
    }
}

// (T)s[j] by truncation, stored the way tnr_load reads
template <typename T, bool VEC, int N>
__device__ __forceinline__ void tnr_store(uint8_t* p, const float (&s)[N])
{
    if constexpr (VEC) {
        constexpr int PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
        unsigned w[N / PER] = {};
#pragma unroll
        for (int j = 0; j < N; ++j) w[j / PER] |= (unsigned)(T)s[j] << (BITS * (j % PER));
        if constexpr (N / PER == 4) *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
        else *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) reinterpret_cast<T*>(p)[j] = (T)s[j];
    }
}

// luma columns [x0, x0 + PX) of rows y0 and y1 and chroma columns [x0 / 2, (x0 + PX) / 2) of row cy, of output frame `out` whose centre is
// the batch's frame `centre`
template <typename T, bool VEC, int PX>
__device__ __forceinline__ void tnr_cell(const TemporalNRArgs& a, int out, int centre, int y0, int y1, int cy, int x0)
{
    constexpr int PC = PX / 2;
    struct Samples { unsigned y[2][PX], u[PC], v[PC]; };
    const long long xY = (long long)x0 * (int)sizeof(T), xC = (long long)(x0 >> 1) * (int)sizeof(T);
    const long long sY0 = (long long)y0 * a.src_pitchY + xY, sY1 = (long long)y1 * a.src_pitchY + xY, sC = (long long)cy * a.src_pitchUV + xC;
    auto load = [&](int f, Samples& s) {
        const long long oY = (long long)f * a.src_strideY, oC = (long long)f * a.src_strideUV;
        tnr_load<T, VEC>(a.srcY + oY + sY0, s.y[0]);
        tnr_load<T, VEC>(a.srcY + oY + sY1, s.y[1]);
        tnr_load<T, VEC>(a.srcU + oC + sC, s.u);
        tnr_load<T, VEC>(a.srcV + oC + sC, s.v);
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
    tnr_store<T, VEC>(a.dstY + oY + (long long)y0 * a.dst_pitchY, sumY[0]);
    tnr_store<T, VEC>(a.dstY + oY + (long long)y1 * a.dst_pitchY, sumY[1]);
    tnr_store<T, VEC>(a.dstU + oC, sumU);
    tnr_store<T, VEC>(a.dstV + oC, sumV);
}

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
        if (x0 + PX <= a.W) { tnr_cell<T, true, PX>(a, out, centre, y0, y1, cy, x0); return; }
#pragma unroll 1
        for (int x = x0; x < a.W; x += 2) tnr_cell<T, false, 2>(a, out, centre, y0, y1, cy, x);
    } else {
        tnr_cell<T, false, 2>(a, out, centre, y0, y1, cy, x0);
    }
}

hipError_t launch_temporal_nr(hipStream_t st, const TemporalNRArgs& a, int nout)
{
    if (nout <= 0) return hipSuccess;
    if ((a.es != 1 && a.es != 2) || a.d < 0 || a.d > 63 || a.W <= 0 || a.H <= 0 || (a.W & 1) || (a.H & 1)) return hipErrorInvalidValue;
    const int px = a.vec ? 16 / a.es : 2;
    const long long cells_per_row = (a.W + px - 1) / px, cells = cells_per_row * (a.H >> 1);
    const long long blocks_per_frame = (cells + 255) / 256;
    if (cells > 0x7FFFFF00LL || blocks_per_frame * nout > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    dim3 grid((unsigned)(blocks_per_frame * nout)), block(256);
    if (a.es == 1 && a.vec) hipLaunchKernelGGL((temporal_nr_kernel<uint8_t, true>), grid, block, 0, st, a, (int)cells_per_row, (int)blocks_per_frame);
    else if (a.es == 1) hipLaunchKernelGGL((temporal_nr_kernel<uint8_t, false>), grid, block, 0, st, a, (int)cells_per_row, (int)blocks_per_frame);
    else if (a.vec) hipLaunchKernelGGL((temporal_nr_kernel<uint16_t, true>), grid, block, 0, st, a, (int)cells_per_row, (int)blocks_per_frame);
    else hipLaunchKernelGGL((temporal_nr_kernel<uint16_t, false>), grid, block, 0, st, a, (int)cells_per_row, (int)blocks_per_frame);
    return hipGetLastError();
}

} // namespace amt
