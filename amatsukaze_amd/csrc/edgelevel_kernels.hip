// edgelevel_kernels.hip -- the edge level of DESIGN.md section 6g ("parity unpinned": KEdgeLevel belongs to AviSynthCUDAFilters, whose
// source is not in the reference tree; only the server's script text calls it, Misc.cs:1435) on planar LSB planes in HBM: integer, exact.
// Per interior luma pixel c = s[y][x], with T = threshold << (bits - 8):
//   the line L is the column s[y-2 .. y+2][x] where its range exceeds the range of the row s[y][x-2 .. x+2], else the row;
//   mx, mn, rng = mx - mn of L, step = the largest difference of neighbours in L;
//   rng <= T (flat), 4 step >= 3 rng (sharp already) or 8 step <= 3 rng (too blurred): out = c;
//   else e = c + (((c - (mx + mn >> 1)) * strength) >> 4) clamped into [mn, mx], then into [n[r - 1], n[9 - r]] of the sorted 3 x 3
//   around the pixel where repair = r > 0.
// The two outermost rows and columns, and both chroma planes, are copied.
// By its bytes a whole-frame copy, so the luma plane is read about once: a wave owns a strip of kEdgeStripRows output rows of a span of
// 64 x 16 bytes and slides a window of five rows down it in registers -- one 16-byte load per lane and new row, requested one row ahead
// of its use; a strip's four halo rows are read by two strips.  The two containers to the left and right of a lane's 16 bytes come
// from the neighbouring lanes' registers (v_mov_b32_dpp wave_shr:1 / wave_shl:1; no LDS); only lane 0 and lane 63 load theirs, as one
// pair, and the lane that holds a row's last containers, fewer than 16 bytes of them, loads and stores container by container.
// Where edgelevel_vec16 does not hold a lane takes one pixel and loads its thirteen containers one by one.  repair is a wave-uniform
// argument that picks one of five row loops, outside the pixel work: five forms of the cell in each of the four kernels ({8-bit,
// 16-bit} x {16-byte lanes, container by container}) instead of twenty kernels.  Chroma rows are copied by further blocks of the same
// launch, a wave a row.  Frame and strip offsets are 64-bit products on the scalar unit; rows are stepped pointers.  No LDS, no
// atomics, no scratch.  The rule's text is edgelevel_body.h's.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "kernels.hpp"
#include "edgelevel_body.h"

namespace amt {

namespace {

// what a lane has asked for of a row: its 16 bytes, and at a wave's seams the pair of containers beside them
struct EdgeRaw { uint4 v; uint32_t l, r; };

// v, which is the same in every lane, held in scalar registers: frame and row offsets are 64-bit products that stay on the scalar unit
// instead of being folded, with a lane's column, into one 64-bit multiply-add per lane
__device__ __forceinline__ long long edge_uniform(long long v)
{
    return (long long)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v) |
                       (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32)) << 32);
}

// rows [ys, ye) of the containers [xs, xs + 64 * 16 / es) of one frame's luma plane, 16 bytes per lane.  s / d: row 0 of the frame
template <typename T, int REP>
__device__ __forceinline__ void edge_strip_vec(const uint8_t* s, uint8_t* d, int spitch, int dpitch, int W, int H, int ys, int ye, int xs, int lane,
                                               int thresh, int strength)
{
    constexpr int ES = (int)sizeof(T), PX = 16 / ES, PER = 4 / ES, BITS = 8 * ES;
    const int x0 = xs + lane * PX;                                                       // the lane's first container
    const bool full = x0 + PX <= W, part = x0 < W && !full;
    // no lane with the left / right neighbours in its registers, and neighbours there are
    const bool seam_l = lane == 0 && x0 > 0, seam_r = lane == 63 && x0 + PX < W;
    // all-ones over the containers of the plane's two outermost columns, which keep the source's
    uint32_t keep[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < PX; ++j)
        if (x0 + j < 2 || x0 + j >= W - 2) keep[j / PER] |= ((1u << BITS) - 1) << (BITS * (j % PER));

    auto load = [&](const uint8_t* p) {                                                  // p: the row's first byte
        EdgeRaw q = {uint4{0, 0, 0, 0}, 0, 0};
        if (full) {
            q.v = *reinterpret_cast<const uint4*>(p + x0 * ES);
        } else if (part) {
            uint32_t t[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < PX; ++j)
                if (x0 + j < W) t[j / PER] |= (uint32_t)reinterpret_cast<const T*>(p)[x0 + j] << (BITS * (j % PER));
            q.v = uint4{t[0], t[1], t[2], t[3]};
        }
        // containers x0 - 2, x0 - 1 and x0 + PX, x0 + PX + 1: W and x0 are even, so a pair lies inside the row with its first container
        if (seam_l) q.l = ES == 1 ? (uint32_t)*reinterpret_cast<const uint16_t*>(p + x0 - 2) << 16 : *reinterpret_cast<const uint32_t*>(p + (x0 - 2) * 2);
        if (seam_r) q.r = ES == 1 ? (uint32_t)*reinterpret_cast<const uint16_t*>(p + x0 + PX) : *reinterpret_cast<const uint32_t*>(p + (x0 + PX) * 2);
        return q;
    };
    auto finish = [&](const EdgeRaw& q) {
        const uint32_t l = edge_from_left(q.v.w), r = edge_from_right(q.v.x);
        return EdgeRow{{seam_l ? q.l : l, q.v.x, q.v.y, q.v.z, q.v.w, seam_r ? q.r : r}};
    };

    // row `row` enters the window at the bottom, and output row `row - 2` is its middle.  A row outside the plane is not loaded: what
    // the window holds in its place is read only by the cell of a border row, whose result is not kept
    EdgeRow w[5] = {};
    EdgeRaw next = {uint4{0, 0, 0, 0}, 0, 0};
    const uint8_t* sp = s + edge_uniform((long long)(ys - 2) * spitch);                              // row ys - 2: not formed into an address above the plane
    uint8_t* dp = d + edge_uniform((long long)ys * dpitch);                                         // (the lane's x0 * ES is added where it stores)
    if (ys >= 2) next = load(sp);
#pragma unroll 1
    for (int row = ys - 2; row < ye + 2; ++row) {
        w[0] = w[1]; w[1] = w[2]; w[2] = w[3]; w[3] = w[4];
        w[4] = finish(next);
        sp += spitch;
        if (row + 1 >= 0 && row + 1 < H && row + 1 < ye + 2) next = load(sp);             // the next row is on its way during this row's pixels
        const int y = row - 2;
        if (y >= ys) {
            const uint32_t c[4] = {w[2].d[1], w[2].d[2], w[2].d[3], w[2].d[4]};
            uint32_t o[4] = {c[0], c[1], c[2], c[3]};
            if (y >= 2 && y < H - 2) {
                const uint4 e = edge_cell<T, REP>(w, thresh, strength);
                o[0] = (c[0] & keep[0]) | (e.x & ~keep[0]); o[1] = (c[1] & keep[1]) | (e.y & ~keep[1]);
                o[2] = (c[2] & keep[2]) | (e.z & ~keep[2]); o[3] = (c[3] & keep[3]) | (e.w & ~keep[3]);
            }
            if (full) {
                *reinterpret_cast<uint4*>(dp + x0 * ES) = uint4{o[0], o[1], o[2], o[3]};
            } else if (part) {
#pragma unroll
                for (int j = 0; j < PX; ++j)
                    if (x0 + j < W) reinterpret_cast<T*>(dp)[x0 + j] = (T)(o[j / PER] >> (BITS * (j % PER)));
            }
            dp += dpitch;
        }
    }
}

// the same rows and containers, a lane a pixel
template <typename T, int REP>
__device__ __forceinline__ void edge_strip_narrow(const uint8_t* s, uint8_t* d, int spitch, int dpitch, int W, int H, int ys, int ye, int xs, int lane,
                                                  int thresh, int strength)
{
    constexpr int ES = (int)sizeof(T);
    const int xe = min(xs + kEdgeSpanBytes / ES, W);
    const uint8_t* sp = s + edge_uniform((long long)ys * spitch);
    uint8_t* dp = d + edge_uniform((long long)ys * dpitch);
#pragma unroll 1
    for (int y = ys; y < ye; ++y, sp += spitch, dp += dpitch) {
        const bool inner = y >= 2 && y < H - 2;
        // rows y - 2 .. y + 2, each a scalar pointer (not dereferenced where the row lies outside the plane)
        const long long one = edge_uniform((long long)spitch), two = edge_uniform(2ll * spitch);
        const T *r0 = reinterpret_cast<const T*>(sp - two), *r1 = reinterpret_cast<const T*>(sp - one), *r2 = reinterpret_cast<const T*>(sp),
                *r3 = reinterpret_cast<const T*>(sp + one), *r4 = reinterpret_cast<const T*>(sp + two);
#pragma unroll 1
        for (int x = xs + lane; x < xe; x += 64) {
            int out = r2[x];
            if (inner && x >= 2 && x < W - 2) {
                const int h[5] = {r2[x - 2], r2[x - 1], out, r2[x + 1], r2[x + 2]};
                const int v[5] = {r0[x], r1[x], out, r3[x], r4[x]};
                const int u[3] = {r1[x - 1], v[1], r1[x + 1]}, n[3] = {r3[x - 1], v[3], r3[x + 1]};
                out = edge_pixel<int, REP>(h, v, u, n, thresh, strength);
            }
            reinterpret_cast<T*>(dp)[x] = (T)out;
        }
    }
}

} // namespace

// VEC: edgelevel_vec16 (lane_rule.h).  units: luma units of a frame, `spans` of them side by side; luma_blocks: the blocks that take them
template <typename T, bool VEC>
__global__ __launch_bounds__(256)
void edgelevel_kernel(EdgeLevelArgs a, int spans, int units, int luma_blocks, int nframes)
{
    constexpr int ES = (int)sizeof(T);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x;
    if (b < luma_blocks) {
        const int u = b * 4 + wave;
        if (u >= units) return;
        const int strip = u / spans, span = u - strip * spans;
        const int ys = strip * kEdgeStripRows, ye = min(ys + kEdgeStripRows, a.H), xs = span * (kEdgeSpanBytes / ES);
#pragma unroll 1
        for (long long f = blockIdx.y; f < nframes; f += gridDim.y) {
            const uint8_t* s = a.srcY + edge_uniform(f * a.src_strideY);
            uint8_t* d = a.dstY + edge_uniform(f * a.dst_strideY);
            auto rows = [&](auto rep) {
                if constexpr (VEC) edge_strip_vec<T, decltype(rep)::value>(s, d, a.src_pitchY, a.dst_pitchY, a.W, a.H, ys, ye, xs, lane, a.thresh, a.strength);
                else edge_strip_narrow<T, decltype(rep)::value>(s, d, a.src_pitchY, a.dst_pitchY, a.W, a.H, ys, ye, xs, lane, a.thresh, a.strength);
            };
            if (a.repair == 0) rows(std::integral_constant<int, 0>());
            else if (a.repair == 1) rows(std::integral_constant<int, 1>());
            else if (a.repair == 2) rows(std::integral_constant<int, 2>());
            else if (a.repair == 3) rows(std::integral_constant<int, 3>());
            else rows(std::integral_constant<int, 4>());
        }
    } else {
        // a chroma row: U's rows, then V's
        const int r = (b - luma_blocks) * 4 + wave, hc = a.H >> 1;
        if (r >= 2 * hc) return;
        const bool second = r >= hc;
        const int y = second ? r - hc : r, nb = (a.W >> 1) * ES;
        const uint8_t* sp = (second ? a.srcV : a.srcU) + (long long)y * a.src_pitchUV;
        uint8_t* dp = (second ? a.dstV : a.dstU) + (long long)y * a.dst_pitchUV;
#pragma unroll 1
        for (long long f = blockIdx.y; f < nframes; f += gridDim.y) {
            const uint8_t* s = sp + edge_uniform(f * a.src_strideUV);
            uint8_t* d = dp + edge_uniform(f * a.dst_strideUV);
            if constexpr (VEC) {
                for (int x = lane * 16; x + 16 <= nb; x += 64 * 16) *reinterpret_cast<uint4*>(d + x) = *reinterpret_cast<const uint4*>(s + x);
                for (int k = (nb & ~15) / ES + lane; k < nb / ES; k += 64) reinterpret_cast<T*>(d)[k] = reinterpret_cast<const T*>(s)[k];
            } else {
                for (int k = lane; k < nb / ES; k += 64) reinterpret_cast<T*>(d)[k] = reinterpret_cast<const T*>(s)[k];
            }
        }
    }
}

hipError_t launch_edgelevel(hipStream_t st, const EdgeLevelArgs& a, int nframes)
{
    if (nframes <= 0) return hipSuccess;
    EdgeLevelGrid g;
    if (!edgelevel_grid(a, nframes, g)) return hipErrorInvalidValue;
    const dim3 block(256);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, g.grid, block, 0, st, a, g.spans, g.units, g.luma_blocks, nframes); };
    with_sample_type(a.es == 1 ? 8 : 16, [&](auto pix) {
        using T = decltype(pix);
        if (a.vec) go(edgelevel_kernel<T, true>);
        else go(edgelevel_kernel<T, false>);
    });
    return hipGetLastError();
}

} // namespace amt
