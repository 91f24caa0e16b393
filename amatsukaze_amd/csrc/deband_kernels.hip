// deband_kernels.hip -- the deband of DESIGN.md section 6f ("parity unpinned": KDeband belongs to AviSynthCUDAFilters, whose source is not
// in the reference tree; only the server's script text calls it, Misc.cs:1431) on planar LSB planes in HBM: integer, exact.  Per pixel
// (x, y) of a plane with the table's (dx, dy), |dx|, |dy| <= lim(x, y):
//   p0 = s[y + dy][x + dx], p1 = s[y - dy][x - dx], p2 = s[y + dx][x - dy], p3 = s[y - dx][x + dy], c = s[y][x];
//   sample 0: avg = p0; 1: (p0 + p1 + 1) >> 1; 2: (p0 + p1 + p2 + p3 + 2) >> 2;
//   out = avg where |avg - c| <= thresh (blur_first, and sample 0), or where every |p_i - c| <= thresh (not blur_first); else c.
// A per-pixel random gather within +-31 rows and columns: as global loads every wave instruction would touch up to 64 cache lines, so
// the gather runs on LDS.  A 256-thread workgroup owns a tile of kDebandTileW x kDebandTileH output samples of one plane of one frame.
// It stages the tile's rows [y0 - R, y0 + TH + R) and columns [x0 - R, x0 + TW + R), clipped to the plane and begun at a multiple of 16
// bytes of the row, with aligned 16-byte loads where deband_vec16 holds (a row's last containers, and everything where it does not,
// go container by container), ten loads of a lane in flight before its first LDS store; one barrier; then a lane takes 16 bytes of
// an output row: the 16 / es entries of dx and of dy with one vector load each (the tables are the object's own, their rows padded to
// 16; a step's entries are requested one step ahead, the first step's before the staging), its centre samples with one 16-byte LDS read, every
// reference with one container-wide LDS read at centre + dy * pitch + dx -- a 24-bit multiply, the pitch a constant -- and one
// 16-byte store.  Sums of four 16-bit containers are formed in 32-bit registers, one pixel each: nothing is packed into halves.
// sample and blur_first are wave-uniform arguments that pick one of five row loops, outside the pixel work: five forms of the cell
// in each of the four kernels ({8-bit, 16-bit} x {16-byte lanes, container by container}) instead of twenty kernels, and the
// staging, which is most of the kernel's text, exists once per kernel.  Frame offsets are 64-bit; row offsets are formed from 24-bit
// products.  The cell, the table load and the row offsets stand in deband_body.h, which deband_surface_kernels.hip (decoder surfaces in
// kind) compiles too.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "kernels.hpp"
#include "deband_body.h"

namespace amt {

// VEC: deband_vec16 (lane_rule.h).  tilesY / tilesC: tiles of the luma plane / of one chroma plane, tiles_xY / tiles_xC of them in a row
template <typename T, bool VEC>
__global__ __launch_bounds__(256)
void deband_kernel(DebandArgs a, int tilesY, int tiles_xY, int tilesC, int tiles_xC, int nframes)
{
    constexpr int ES = (int)sizeof(T), PX = 16 / ES, PER = 4 / ES, BITS = 8 * ES, PITCH = deband_lds_pitch(ES);
    constexpr int LPR = kDebandTileW / PX, RPS = 256 / LPR;             // lanes of an output row, rows of a step
    constexpr int LPS = ES == 1 ? 16 : 32, RPP = 256 / LPS;             // lanes of a staged row, rows of a staging pass
    __shared__ __attribute__((aligned(16))) uint8_t lds[deband_lds_bytes(ES)];
    const int tid = threadIdx.x;
    // (blockIdx is wave-uniform: the plane's arguments are picked with selects on the scalar unit)
    const int b = blockIdx.x;
    const int plane = b < tilesY ? 0 : b < tilesY + tilesC ? 1 : 2;
    const int r = b - (plane == 0 ? 0 : plane == 1 ? tilesY : tilesY + tilesC);
    const DebandPlaneArgs pa = plane == 0 ? a.plane[0] : plane == 1 ? a.plane[1] : a.plane[2];
    const int across = plane ? tiles_xC : tiles_xY;
    const int ty = r / across, tx = r - ty * across;
    const int x0 = tx * kDebandTileW, y0 = ty * kDebandTileH;
    const int W = pa.W, H = pa.H, R = pa.R;
    // the staged span: columns [xs, sx1) of rows [sy0, sy1); LDS column 0 is column ox of the plane, a multiple of 16 bytes
    const int xs = max(x0 - R, 0), ox = xs & ~(PX - 1), sx1 = min(x0 + kDebandTileW + R, W);
    const int sy0 = max(y0 - R, 0), nrows = min(y0 + kDebandTileH + R, H) - sy0;
    // the lane's cell of an output row
    const int lc = tid & (LPR - 1), lr = tid / LPR;
    const int x = x0 + lc * PX;
    const unsigned thresh = (unsigned)a.thresh;
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
        if constexpr (VEC) {
            // a lane stages 16 bytes: LPS lanes to a row (a row is at most 13 / 25 pieces at 8 / 16 bits), RPP rows to a pass, and
            // kStageBatch passes' loads in flight before the first is stored: a tile is two or three round trips to memory, not twenty
            const int piece = tid & (LPS - 1), row0 = tid / LPS;
            const int first = ox + piece * PX;                          // the piece's first column
            if (first < sx1) {
                const uint8_t* g = src + deband_rows(row0, pa.src_pitch) + (long long)first * ES;
                uint8_t* l = lds + __umul24(row0, PITCH) + piece * 16;
                const long long gstep = (long long)RPP * pa.src_pitch;
                if (first + PX <= W) {
#pragma unroll 1
                    for (int row = row0; row < nrows; row += RPP * kStageBatch, g += kStageBatch * gstep, l += kStageBatch * RPP * PITCH) {
                        uint4 v[kStageBatch];
                        // (a pass behind the last row stages the last row once more: selects and no branches, so that every load is
                        // issued before the first store waits; the offsets are stepped, not multiplied: one scalar stride)
                        long long go = 0;
#pragma unroll
                        for (int i = 0; i < kStageBatch; ++i) {
                            v[i] = *reinterpret_cast<const uint4*>(g + go);
                            go += row + (i + 1) * RPP < nrows ? gstep : 0ll;
                        }
                        int lo = 0;
#pragma unroll
                        for (int i = 0; i < kStageBatch; ++i) {
                            *reinterpret_cast<uint4*>(l + lo) = v[i];
                            lo += row + (i + 1) * RPP < nrows ? RPP * PITCH : 0;
                        }
                    }
                } else {
                    // the row's last containers: fewer than a piece
#pragma unroll 1
                    for (int row = row0; row < nrows; row += RPP, g += gstep, l += RPP * PITCH)
#pragma unroll 1
                        for (int k = 0; first + k < W; ++k) reinterpret_cast<T*>(l)[k] = reinterpret_cast<const T*>(g)[k];
                }
            }
        } else {
            // a lane stages a container: a wave to a row, 4 rows to a pass
            const int col0 = xs + (tid & 63), row0 = tid >> 6;
            const uint8_t* g = src + deband_rows(row0, pa.src_pitch);
            uint8_t* l = lds + __umul24(row0, PITCH);
            const long long gstep = 4ll * pa.src_pitch;
#pragma unroll 1
            for (int row = row0; row < nrows; row += 4, g += gstep, l += 4 * PITCH)
#pragma unroll 1
                for (int col = col0; col < sx1; col += 64) reinterpret_cast<T*>(l)[col - ox] = reinterpret_cast<const T*>(g)[col];
        }
        __syncthreads();

        if (x < W) {
            const uint8_t* centre = lds + __umul24(yfirst - sy0, PITCH) + (x - ox) * ES;
            const int8_t *tdx = tdx0, *tdy = tdy0;
            uint8_t* d = pa.dst + f * pa.dst_stride + (long long)y0 * pa.dst_pitch + deband_rows(lr, pa.dst_pitch) + (long long)x * ES;
            const long long dstep = (long long)RPS * pa.dst_pitch;
            auto rows = [&](auto ns, auto bf) {
                DebandOffsets<PX> cur = first_offsets;
#pragma unroll 1
                for (int y = yfirst; y < yend; y += RPS, centre += RPS * PITCH, tdx += tstep, tdy += tstep, d += dstep) {
                    // the next step's entries are on their way while this step's pixels are worked on
                    DebandOffsets<PX> next = cur;
                    if (y + RPS < yend) next = deband_offsets<PX>(tdx + tstep, tdy + tstep);
                    unsigned out[4];
                    deband_cell<T, decltype(ns)::value, decltype(bf)::value>(centre, cur.dx, cur.dy, thresh, out);
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
            if (a.sample == 0) rows(I1(), std::true_type());
            else if (a.sample == 1) { if (a.blur_first) rows(I2(), std::true_type()); else rows(I2(), std::false_type()); }
            else { if (a.blur_first) rows(I4(), std::true_type()); else rows(I4(), std::false_type()); }
        }
        __syncthreads();                                                // the next frame's staging overwrites what these rows read
    }
}

hipError_t launch_deband(hipStream_t st, const DebandArgs& a, int nframes)
{
    if (nframes <= 0) return hipSuccess;
    DebandGrid g;
    if (!deband_grid(a, nframes, g)) return hipErrorInvalidValue;
    const dim3 block(256);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, g.grid, block, 0, st, a, g.tiles[0], g.tiles_x[0], g.tiles[1], g.tiles_x[1], nframes); };
    with_sample_type(a.es == 1 ? 8 : 16, [&](auto pix) {
        using T = decltype(pix);
        if (a.vec) go(deband_kernel<T, true>);
        else go(deband_kernel<T, false>);
    });
    return hipGetLastError();
}

} // namespace amt
