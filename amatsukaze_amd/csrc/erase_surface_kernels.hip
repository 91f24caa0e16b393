// erase_surface_kernels.hip -- logo erase (Delogo) on decoder surfaces where they lie: NV12, P010 / P012, planar MSB.
//
// delogo_kernel (erase_scan_kernels.hip) takes planar LSB planes.  A transcode host keeps its pictures in the decoder's layout from the
// hardware decoder to the hardware encoder, so this kernel reads and writes CONTAINERS: sample = container >> shift on the way in
// (shift = 16 - bits for MSB-aligned input, else 0), container = result << shift on the way out (the low bits of a rewritten MSB
// container are zero, which is what P010 specifies), and an interleaved chroma row U0 V0 U1 V1 ... is one run of 2 * wUV containers
// whose even members take the U coefficients and whose odd members take the V coefficients -- a frame has h + hUV rows of work
// instead of h + 2 * hUV.  Planar LSB surfaces are ordinary planes and go to delogo_kernel: the launcher refuses them.  (This kernel
// computes them correctly -- interleaved = 0, shift = 0 -- but on a batch that fills the device its one-row-per-wave shape is 37-68 %
// slower than delogo_kernel's: DESIGN.md section 4, profiles/delogo_unify.json.)  Both share delogo_body.h.
//
// Shaped like delogo_kernel: one workgroup = kSurfRows consecutive rectangle rows x up to kSurfFrames consecutive frames, the row's logo
// coefficients (8 B per sample against 2 * es B of frame traffic) loaded once per group and kept in registers, all live frames' loads
// issued before the first use.  Unlike it, a wave owns ONE row (16 waves per workgroup, not 4 that loop over 4 rows each): everything
// about a row -- its plane, fades, pointers -- is then wave-uniform and lives in scalar registers once, and a 256 x 128 rectangle of 64
// frames puts 1536 waves on the device instead of 384.  The pass is an HBM-bound read-modify-write of the rectangle.  A lane moves 4, 2 or 1
// containers, decided per plane kind by the launcher from the alignment of base, stride, pitch, origin and row length (every access is
// naturally aligned); the MSB shifts are packed 16-bit operations on the loaded dwords.  What is not rewritten is not touched: nothing
// outside the rectangle, no odd last chroma row in field mode, no frame with fades {0, 0} when the host says fade 0 is the identity
// (zero_identity).  No LDS, no scratch.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>

#include "delogo_body.h"
#include "kernels.hpp"

namespace amt {

constexpr int kSurfRows = 16;          // rectangle rows per workgroup (delogo_kernel's shape)
constexpr int kSurfThreads = 64 * kSurfRows;      // a wave per row
constexpr int kSurfFrames = 8;         // frames a workgroup walks through with the row's coefficients in registers

// the coefficients of containers c .. c + N - 1 of a row.  Plain rows (luma, planar chroma): A[c + k] and B[c + k] = A[boff + c + k].
// Interleaved chroma (il): container 2x takes U's (A[x], B[x]) and container 2x + 1 takes V's, voff floats behind U's
template <int N>
__device__ __forceinline__ void row_coefficients(const float* __restrict__ A, int boff, int voff, bool il, int c, float (&a)[N], float (&b)[N])
{
    const int x = c >> 1;
    if constexpr (N == 4) {
        if (il) {
            const float2 au = *reinterpret_cast<const float2*>(A + x), bu = *reinterpret_cast<const float2*>(A + boff + x);
            const float2 av = *reinterpret_cast<const float2*>(A + voff + x), bv = *reinterpret_cast<const float2*>(A + voff + boff + x);
            a[0] = au.x; a[1] = av.x; a[2] = au.y; a[3] = av.y;
            b[0] = bu.x; b[1] = bv.x; b[2] = bu.y; b[3] = bv.y;
        } else {
            const float4 av = *reinterpret_cast<const float4*>(A + c), bv = *reinterpret_cast<const float4*>(A + boff + c);
            a[0] = av.x; a[1] = av.y; a[2] = av.z; a[3] = av.w;
            b[0] = bv.x; b[1] = bv.y; b[2] = bv.z; b[3] = bv.w;
        }
    } else if constexpr (N == 2) {
        if (il) {
            a[0] = A[x]; a[1] = A[voff + x];
            b[0] = A[boff + x]; b[1] = A[voff + boff + x];
        } else {
            const float2 av = *reinterpret_cast<const float2*>(A + c), bv = *reinterpret_cast<const float2*>(A + boff + c);
            a[0] = av.x; a[1] = av.y;
            b[0] = bv.x; b[1] = bv.y;
        }
    } else {
        const int i = il ? x + ((c & 1) ? voff : 0) : c;
        a[0] = A[i];
        b[0] = A[boff + i];
    }
}

// one rectangle row of `rowlen` containers (a multiple of N) in the frames of `live` (bit k = frame f0 + k): srow / row = the row in
// frame f0 of the source / destination batch, stride = containers between frames
template <typename C, int N>
__device__ __forceinline__ void delogo_surface_row(const C* srow, C* row, long long stride, int rowlen, const float* __restrict__ A, int boff,
                                                   int voff, bool il, const float (&fd)[kSurfFrames], unsigned live, float maxv, int shift,
                                                   int lane)
{
    typedef Run<C, N> R;
    typedef typename R::type run_t;
    for (int c = N * lane; c < rowlen; c += 64 * N) {
        float a[N], b[N];
        row_coefficients<N>(A, boff, voff, il, c, a, b);
        run_t v[kSurfFrames];                                   // all live frames' loads in flight before the first use
#pragma unroll
        for (int k = 0; k < kSurfFrames; ++k)
            if ((live >> k) & 1u) v[k] = *reinterpret_cast<const run_t*>(srow + (long long)k * stride + c);
#pragma unroll
        for (int k = 0; k < kSurfFrames; ++k) {
            if (!((live >> k) & 1u)) continue;
            float s[N], r[N];
            R::get(v[k], shift, s);
#pragma unroll
            for (int j = 0; j < N; ++j) r[j] = delogo_px(s[j], a[j], b[j], maxv, fd[k]);
            *reinterpret_cast<run_t*>(row + (long long)k * stride + c) = R::pack(r, shift);
        }
    }
}

struct DelogoSurfaceArgs {
    const void *sY, *sU, *sV;              // the rectangle's first container in picture 0 of the source batch (interleaved: sU = its first U V
                                           // pair in the UV plane, sV unused)
    void *Y, *U, *V;                       // ... of the destination batch, laid out like the source (the same planes for the in-place call)
    long long strideY, strideUV;           // CONTAINERS between pictures
    int pitchY, pitchUV;                   // containers between rows
    int w, h, wUV, hUV;                    // the rectangle in the luma plane and in a chroma plane, in samples
    int uvparity;                          // (imgy / 2) % 2: which field a chroma row of the rectangle belongs to
    int interleaved, shift;
    int nY, nC;                            // containers a lane moves in a luma / chroma row: 4, 2 or 1
};

template <typename container_t>
__global__ __launch_bounds__(kSurfThreads)
void delogo_surfaces_kernel(DelogoSurfaceArgs s, const float* __restrict__ planes, float maxv, const float2* __restrict__ fades, int nframes,
                            int zero_identity)
{
    typedef container_t C;
    const int f0 = blockIdx.y * kSurfFrames;
    const int f1 = min(nframes, f0 + kSurfFrames);
    const int ysz = s.w * s.h, csz = s.wUV * s.hUV;                             // (a logo's planes are far below 2^31 floats)
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // a wave per row: everything about the row is scalar
    // per frame of the group, as bit k of a mask: field mode (fadeT != fadeB); fades {0, 0} where fade 0 is the identity.  Frames behind
    // the batch's end read the last frame's fades and are never live
    const int nf = f1 - f0;
    const unsigned valid = (1u << nf) - 1u;
    unsigned field = 0, zero = 0;
#pragma unroll
    for (int k = 0; k < kSurfFrames; ++k) {
        const float2 p = fades[f0 + min(k, nf - 1)];
        field |= (p.x != p.y ? 1u : 0u) << k;
        zero |= (p.x == 0.0f && p.y == 0.0f ? 1u : 0u) << k;
    }
    if (!zero_identity) zero = 0;
    // a group whose frames all carry fade {0, 0} has nothing to rewrite: leave before the coefficient rows are fetched
    if (!(valid & ~zero)) return;
    const int crows = s.interleaved ? s.hUV : 2 * s.hUV;
    const int r = blockIdx.x * kSurfRows + wv;
    if (r >= s.h + crows) return;
    const int pl = r < s.h ? 0 : (!s.interleaved && (r - s.h) >= s.hUV ? 2 : 1);
    const int y = pl == 0 ? r : r - s.h - (pl - 1) * s.hUV;
    // the planar rule (U and V of an interleaved row share fade, parity and skip): field mode leaves an odd last chroma row alone and
    // gives a row its field's fade -- luma rows by their own parity, chroma rows by the parity of the logo's position
    const bool odd_last = pl != 0 && y >= 2 * (s.hUV / 2);
    const bool top = pl == 0 ? (y & 1) == 0 : (y & 1) == s.uvparity;
    const unsigned live = valid & ~zero & ~(odd_last ? field : 0u);
    if (!live) return;
    float fd[kSurfFrames];
#pragma unroll
    for (int k = 0; k < kSurfFrames; ++k) {
        const float2 p = fades[f0 + min(k, nf - 1)];
        fd[k] = (top || !((field >> k) & 1u)) ? p.x : p.y;                   // (frame mode: fadeT)
    }
    // the row in frame f0, its length in containers and its coefficient rows: luma, an interleaved U V row, or a row of a planar U
    // or V plane (MSB-aligned: planar LSB surfaces go to delogo_kernel)
    const bool il = pl != 0 && s.interleaved;
    const long long stride = pl == 0 ? s.strideY : s.strideUV;
    const long long at = (long long)f0 * stride + (long long)y * (pl == 0 ? s.pitchY : s.pitchUV);
    const C* srow = (const C*)(pl == 0 ? s.sY : pl == 2 ? s.sV : s.sU) + at;
    C* row = (C*)(pl == 0 ? s.Y : pl == 2 ? s.V : s.U) + at;
    const int roww = pl == 0 ? s.w : s.wUV;
    const float* A = planes + ((pl == 0 ? 0 : 2 * ysz + (pl - 1) * 2 * csz) + y * roww);
    const int boff = pl == 0 ? ysz : csz, voff = 2 * csz;           // B's rows behind A's; V's rows behind U's (interleaved rows only)
    const int rowlen = il ? 2 * roww : roww;
    const int n = pl == 0 ? s.nY : s.nC;
    if (n == 4) delogo_surface_row<C, 4>(srow, row, stride, rowlen, A, boff, voff, il, fd, live, maxv, s.shift, lane);
    else if (n == 2) delogo_surface_row<C, 2>(srow, row, stride, rowlen, A, boff, voff, il, fd, live, maxv, s.shift, lane);
    else delogo_surface_row<C, 1>(srow, row, stride, rowlen, A, boff, voff, il, fd, live, maxv, s.shift, lane);
}

hipError_t launch_delogo_surfaces(hipStream_t st, int bits, const FrameBatch& src, const PlanesOut& dst, const float* dplanes, EraseGeom g,
                                  int nframes, const float2* dfades, int zero_identity)
{
    if (nframes <= 0) return hipSuccess;
    const int es = src.es, il = src.interleaved ? 1 : 0;
    if ((es != 1 && es != 2) || es != (bits <= 8 ? 1 : 2) || (es == 1 && src.shift) || src.shift < 0 || src.shift > 7) return hipErrorInvalidValue;
    if (!il && !src.shift) return hipErrorInvalidValue;                  // planar LSB surfaces are launch_delogo's
    if (src.strideY % es || src.strideUV % es) return hipErrorInvalidValue;
    // the rectangle's rows lie inside the surface's rows: nothing is read or written behind a row's end
    if (g.imgx < 0 || g.imgy < 0 || g.cx < 0 || g.cy < 0 || g.w <= 0 || g.h <= 0 || g.wUV < 0 || g.hUV < 0 || src.pitchY < g.imgx + g.w ||
        src.pitchUV < (il ? 2 : 1) * (g.cx + g.wUV))
        return hipErrorInvalidValue;
    if (!src.Y || !src.U || (!il && !src.V) || !dst.Y || !dst.U || (!il && !dst.V)) return hipErrorInvalidValue;
    DelogoSurfaceArgs a;
    // an interleaved row holds the pair of chroma sample x at container 2 x
    const long long atY = ((long long)g.imgy * src.pitchY + g.imgx) * es, atC = ((long long)g.cy * src.pitchUV + (long long)g.cx * (il ? 2 : 1)) * es;
    a.sY = (const uint8_t*)src.Y + atY; a.sU = (const uint8_t*)src.U + atC; a.sV = il ? nullptr : (const uint8_t*)src.V + atC;
    a.Y = (uint8_t*)dst.Y + atY; a.U = (uint8_t*)dst.U + atC; a.V = il ? nullptr : (uint8_t*)dst.V + atC;
    a.strideY = src.strideY / es; a.strideUV = src.strideUV / es;
    a.pitchY = src.pitchY; a.pitchUV = src.pitchUV;
    a.w = g.w; a.h = g.h; a.wUV = g.wUV; a.hUV = g.hUV; a.uvparity = g.uvparity;
    a.interleaved = il; a.shift = src.shift;
    // a lane's access of n containers is naturally aligned: the first container's address, stride, pitch and row length are multiples
    // of n * es bytes
    const long long pitchY = (long long)src.pitchY * es, pitchUV = (long long)src.pitchUV * es;
    a.nY = delogo_surface_lane_containers(es, RowsAt{lane_addr(a.sY), 0, src.strideY, pitchY}, RowsAt{lane_addr(a.Y), 0, src.strideY, pitchY},
                                          (long long)g.w * es);
    a.nC = delogo_surface_lane_containers(es, RowsAt{lane_addr(a.sU), lane_addr(a.sV), src.strideUV, pitchUV},
                                          RowsAt{lane_addr(a.U), lane_addr(a.V), src.strideUV, pitchUV}, (il ? 2LL : 1LL) * g.wUV * es);
    const int rows = g.h + (il ? 1 : 2) * g.hUV;
    dim3 grid((unsigned)((rows + kSurfRows - 1) / kSurfRows), (unsigned)((nframes + kSurfFrames - 1) / kSurfFrames)), block(kSurfThreads);
    const float maxv = (float)((1 << bits) - 1);
    with_sample_type(bits, [&](auto px) {
        typedef decltype(px) container_t;
        hipLaunchKernelGGL(delogo_surfaces_kernel<container_t>, grid, block, 0, st, a, dplanes, maxv, dfades, nframes, zero_identity);
    });
    return hipGetLastError();
}

} // namespace amt
