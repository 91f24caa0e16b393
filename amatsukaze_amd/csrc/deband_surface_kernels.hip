// deband_surface_kernels.hip -- the deband of DESIGN.md section 6f on decoder surfaces in kind: NV12, interleaved 16-bit LSB,
// P010 / P012 / P016 (interleaved, MSB-aligned) and planar 16-bit MSB, each with 16-byte lanes and container by container: eight forms.
// The rule, the cell and the shape are the planar kernel's (deband_kernels.hip, deband_body.h): a 256-thread workgroup owns a tile of
// kDebandTileW x kDebandTileH containers of one plane of one frame, stages it with its halo into LDS, one barrier, then a lane takes
// 16 bytes of an output row; luma tiles and chroma tiles in one grid, one launch per call.  What differs:
//   the interleaved UV plane  is walked as ONE plane of `width` containers by height / 2 rows.  U is the even container and V the odd
//       one, and they stay as independent as planes: the object's interleaved table holds U's entry at 2x and V's at 2x + 1, so a lane
//       still loads its 16 / es entries with one vector load of dx and one of dy, and the cell steps 2 containers per unit of a
//       horizontal offset (o0 = dy * ROW + 2 * dx, o2 = dx * ROW - 2 * dy): a reference of a U container is a U container.  The halo
//       is 2 * (radius >> 1) columns, at most 30, and radius >> 1 rows: two arguments where the planar kernel has one R.
//   MSB forms  shift once while they stage -- one packed 16-bit right shift per staged dword, a shift per container on the narrow
//       paths and a row's last containers -- so LDS holds samples and the cell is the LSB cell; the staged halo is about twice the
//       frame, which costs less than shifting at each of the five LDS reads of a pixel.  Stores go through one packed left shift per
//       dword, so every destination container has zero low bits.
// Frame offsets are 64-bit; row offsets and LDS addresses come from 24-bit products.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "kernels.hpp"
#include "pack16.h"
#include "deband_body.h"

namespace amt {

// A workgroup of 256 stages columns [xs, sx1) of nrows rows of a plane of W containers into lds, whose column 0 is the plane's column
// ox = xs rounded down to 16 bytes; src points at the first staged row.  MSB: LDS takes container >> s.  The caller's barrier follows
template <typename T, bool VEC, bool MSB>
__device__ __forceinline__ void deband_surface_stage(uint8_t* lds, const uint8_t* src, int src_pitch, int W, int xs, int ox, int sx1, int nrows, int s)
{
    constexpr int ES = (int)sizeof(T), PX = 16 / ES, PITCH = deband_lds_pitch(ES);
    constexpr int LPS = ES == 1 ? 16 : 32, RPP = 256 / LPS;             // lanes of a staged row, rows of a staging pass
    static_assert(!MSB || ES == 2, "MSB-aligned containers are 16 bits wide");
    const int tid = threadIdx.x;
    if constexpr (VEC) {
        // a lane stages 16 bytes: LPS lanes to a row, RPP rows to a pass, kStageBatch passes' loads in flight before the first is stored
        const int piece = tid & (LPS - 1), row0 = tid / LPS;
        const int first = ox + piece * PX;                              // the piece's first column
        if (first < sx1) {
            const uint8_t* g = src + deband_rows(row0, src_pitch) + (long long)first * ES;
            uint8_t* l = lds + __umul24(row0, PITCH) + piece * 16;
            const long long gstep = (long long)RPP * src_pitch;
            if (first + PX <= W) {
#pragma unroll 1
                for (int row = row0; row < nrows; row += RPP * kStageBatch, g += kStageBatch * gstep, l += kStageBatch * RPP * PITCH) {
                    uint4 v[kStageBatch];
                    // (a pass behind the last row stages the last row once more: selects and no branches)
                    long long go = 0;
#pragma unroll
                    for (int i = 0; i < kStageBatch; ++i) {
                        v[i] = *reinterpret_cast<const uint4*>(g + go);
                        go += row + (i + 1) * RPP < nrows ? gstep : 0ll;
                    }
                    int lo = 0;
#pragma unroll
                    for (int i = 0; i < kStageBatch; ++i) {
                        if constexpr (MSB) v[i] = make_uint4(pk_shr16(v[i].x, s), pk_shr16(v[i].y, s), pk_shr16(v[i].z, s), pk_shr16(v[i].w, s));
                        *reinterpret_cast<uint4*>(l + lo) = v[i];
                        lo += row + (i + 1) * RPP < nrows ? RPP * PITCH : 0;
                    }
                }
            } else {
                // the row's last containers: fewer than a piece
#pragma unroll 1
                for (int row = row0; row < nrows; row += RPP, g += gstep, l += RPP * PITCH)
#pragma unroll 1
                    for (int k = 0; first + k < W; ++k) {
                        const T c = reinterpret_cast<const T*>(g)[k];
                        reinterpret_cast<T*>(l)[k] = MSB ? (T)(c >> s) : c;
                    }
            }
        }
    } else {
        // a lane stages a container: a wave to a row, 4 rows to a pass
        const int col0 = xs + (tid & 63), row0 = tid >> 6;
        const uint8_t* g = src + deband_rows(row0, src_pitch);
        uint8_t* l = lds + __umul24(row0, PITCH);
        const long long gstep = 4ll * src_pitch;
#pragma unroll 1
        for (int row = row0; row < nrows; row += 4, g += gstep, l += 4 * PITCH)
#pragma unroll 1
            for (int col = col0; col < sx1; col += 64) {
                const T c = reinterpret_cast<const T*>(g)[col];
                reinterpret_cast<T*>(l)[col - ox] = MSB ? (T)(c >> s) : c;
            }
    }
}

// VEC: deband_vec16 (lane_rule.h); MSB: containers are samples << a.shift; IL: plane 1 is the interleaved UV plane.
// tilesY / tilesC: tiles of the luma plane / of one chroma plane (IL: of the UV plane), tiles_xY / tiles_xC of them in a row
template <typename T, bool VEC, bool MSB, bool IL>
__global__ __launch_bounds__(256)
void deband_surface_kernel(DebandSurfaceArgs a, int tilesY, int tiles_xY, int tilesC, int tiles_xC, int nframes)
{
    constexpr int ES = (int)sizeof(T), PX = 16 / ES, PER = 4 / ES, BITS = 8 * ES, PITCH = deband_lds_pitch(ES);
    constexpr int LPR = kDebandTileW / PX, RPS = 256 / LPR;             // lanes of an output row, rows of a step
    __shared__ __attribute__((aligned(16))) uint8_t lds[deband_lds_bytes(ES)];
    const int tid = threadIdx.x;
    // (blockIdx is wave-uniform: the plane's arguments are picked with selects on the scalar unit)
    const int b = blockIdx.x;
    const int plane = b < tilesY ? 0 : (IL || b < tilesY + tilesC) ? 1 : 2;
    const int r = b - (plane == 0 ? 0 : plane == 1 ? tilesY : tilesY + tilesC);
    const DebandSurfacePlaneArgs pa = plane == 0 ? a.plane[0] : (IL || plane == 1) ? a.plane[1] : a.plane[2];
    const int across = plane ? tiles_xC : tiles_xY;
    const int ty = r / across, tx = r - ty * across;
    const int x0 = tx * kDebandTileW, y0 = ty * kDebandTileH;
    const int W = pa.W, H = pa.H, RX = pa.RX, RY = pa.RY;
    const int s = MSB ? a.shift : 0;
    // the staged span: columns [xs, sx1) of rows [sy0, sy1); LDS column 0 is column ox of the plane, a multiple of 16 bytes
    const int xs = max(x0 - RX, 0), ox = xs & ~(PX - 1), sx1 = min(x0 + kDebandTileW + RX, W);
    const int sy0 = max(y0 - RY, 0), nrows = min(y0 + kDebandTileH + RY, H) - sy0;
    // the lane's cell of an output row
    const int lc = tid & (LPR - 1), lr = tid / LPR;
    const int x = x0 + lc * PX;
    const unsigned thresh = (unsigned)a.thresh;
    // the row loop: 0 sample 0; 1 / 2 sample 1 with / without blur_first; 3 / 4 sample 2.  One scalar, compared where a loop is picked
    const int mode = a.sample == 0 ? 0 : 2 * a.sample - (a.blur_first ? 1 : 0);
    // the lane's first table entries: the same for every frame, and asked for before anything is staged
    const int yfirst = y0 + lr, yend = min(y0 + kDebandTileH, H);
    const int tstep = RPS * pa.table_pitch;
    const size_t tat = (size_t)__umul24(yfirst, pa.table_pitch) + (size_t)x;
    const int8_t *tdx0 = pa.dx + tat, *tdy0 = pa.dy + tat;
    DebandOffsets<PX> first_offsets = {};
    if (x < W && yfirst < yend) first_offsets = deband_offsets<PX>(tdx0, tdy0);

#pragma unroll 1
    for (long long f = blockIdx.y; f < nframes; f += gridDim.y) {
        const uint8_t* src = pa.src + f * pa.src_stride + (long long)sy0 * pa.src_pitch;
        deband_surface_stage<T, VEC, MSB>(lds, src, pa.src_pitch, W, xs, ox, sx1, nrows, s);
        __syncthreads();

        if (x < W) {
            const uint8_t* centre = lds + __umul24(yfirst - sy0, PITCH) + (x - ox) * ES;
            const int8_t *tdx = tdx0, *tdy = tdy0;
            uint8_t* d = pa.dst + f * pa.dst_stride + (long long)y0 * pa.dst_pitch + deband_rows(lr, pa.dst_pitch) + (long long)x * ES;
            const long long dstep = (long long)RPS * pa.dst_pitch;
            auto rows = [&](auto ns, auto bf, auto step) {
                DebandOffsets<PX> cur = first_offsets;
#pragma unroll 1
                for (int y = yfirst; y < yend; y += RPS, centre += RPS * PITCH, tdx += tstep, tdy += tstep, d += dstep) {
                    // the next step's entries are on their way while this step's pixels are worked on
                    DebandOffsets<PX> next = cur;
                    if (y + RPS < yend) next = deband_offsets<PX>(tdx + tstep, tdy + tstep);
                    unsigned out[4];
                    deband_cell<T, decltype(ns)::value, decltype(bf)::value, decltype(step)::value>(centre, cur.dx, cur.dy, thresh, out);
                    if constexpr (MSB) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) out[i] = pk_shl16(out[i], s);
                    }
                    if (VEC && x + PX <= W) {
                        *reinterpret_cast<uint4*>(d) = make_uint4(out[0], out[1], out[2], out[3]);
                    } else {
#pragma unroll
                        for (int j = 0; j < PX; ++j)
                            if (x + j < W) reinterpret_cast<T*>(d)[j] = (T)(out[j / PER] >> (BITS * (j % PER)));
                    }
                    cur = next;
                }
            };
            using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>; using I4 = std::integral_constant<int, 4>;
            auto modes = [&](auto step) {
                if (mode == 0) rows(I1(), std::true_type(), step);
                else if (mode == 1) rows(I2(), std::true_type(), step);
                else if (mode == 2) rows(I2(), std::false_type(), step);
                else if (mode == 3) rows(I4(), std::true_type(), step);
                else rows(I4(), std::false_type(), step);
            };
            // (the plane is wave-uniform: the UV plane's tiles take the cell whose horizontal step is 2 containers)
            if (IL && plane) modes(I2()); else modes(I1());
        }
        __syncthreads();                                                // the next frame's staging overwrites what these rows read
    }
}

hipError_t launch_deband_surfaces(hipStream_t st, const DebandSurfaceArgs& a, int nframes)
{
    if (nframes <= 0) return hipSuccess;
    DebandGrid g;
    if (!deband_surface_grid(a, nframes, g)) return hipErrorInvalidValue;
    const bool il = a.nplanes == 2, msb = a.shift != 0;
    if (!il && !msb) return hipErrorInvalidValue;                       // planar LSB planes: launch_deband
    if (a.es == 1 && !il) return hipErrorInvalidValue;
    const dim3 block(256);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, g.grid, block, 0, st, a, g.tiles[0], g.tiles_x[0], g.tiles[1], g.tiles_x[1], nframes); };
    auto lanes = [&](auto vec) {
        constexpr bool V = decltype(vec)::value;
        if (a.es == 1) go(deband_surface_kernel<uint8_t, V, false, true>);
        else if (il && !msb) go(deband_surface_kernel<uint16_t, V, false, true>);
        else if (il) go(deband_surface_kernel<uint16_t, V, true, true>);
        else go(deband_surface_kernel<uint16_t, V, true, false>);
    };
    if (a.vec) lanes(std::true_type()); else lanes(std::false_type());
    return hipGetLastError();
}

} // namespace amt
