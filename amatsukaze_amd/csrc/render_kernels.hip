// render_kernels.hip -- the pictures of the cadence decisions (self-specified, "parity unpinned": KFMDeint's source is not in the reference
// tree): field-matched film frames (weave) and bob-deinterlaced video fields, written straight from the source
// frames in HBM.  Per output frame one plan entry: WEAVE takes even rows from picture `top` and odd rows from picture `bottom`;
// BOB_TOP / BOB_BOTTOM keep the even / odd rows of picture n and fill each missing row y with
//     |a - b| <= thresh (and thresh >= 0) ? (a + b + 1) >> 1 : (up + dn + 1) >> 1
// up / dn = rows y - 1 / y + 1 of n (one outside the plane takes the other's value), a / b = row y of the two pictures whose field of that
// parity lies before and after the kept field in time (n - 1 and n for BOB_TOP, n and n + 1 for BOB_BOTTOM).  The rule is symmetric in a
// and b, so the plan names only the picture that is not n (`other`).  Samples are the containers as stored.
// HBM-bound like the weave it is shaped after: one wave per output row, 16 bytes per lane where everything is 16-byte aligned, an
// interpolated row's 2 (4) loads issued together, packed arithmetic; no LDS, no atomics, no scratch.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "kernels.hpp"

namespace amt {

constexpr int kRenderRows = 8;      // rows per workgroup (one wave per row, two rounds)

typedef unsigned short render_us2 __attribute__((ext_vector_type(2)));

// (x + y + 1) >> 1 of every container of a dword
template <int ES> __device__ __forceinline__ uint32_t render_avg(uint32_t x, uint32_t y)
{
    if constexpr (ES == 1) return __builtin_amdgcn_lerp(x, y, 0x01010101u);              // v_lerp_u8: (x + y + (bit 0 of the third operand's byte)) >> 1
    else return (x | y) - (((x ^ y) >> 1) & 0x7FFF7FFFu);                                // no 17th bit: x | y >= (x ^ y) >> 1 in each half, so no borrow crosses
}

// all ones in every container of a dword where |x - y| <= t (t within the container's range)
template <int ES> __device__ __forceinline__ uint32_t render_within(uint32_t x, uint32_t y, uint32_t t)
{
    auto absdiff = [](uint32_t p, uint32_t q) {                                          // per 16-bit half
        const render_us2 pv = __builtin_bit_cast(render_us2, p), qv = __builtin_bit_cast(render_us2, q);
        return __builtin_bit_cast(uint32_t, (render_us2)(__builtin_elementwise_max(pv, qv) - __builtin_elementwise_min(pv, qv)));
    };
    if constexpr (ES == 1) {
        // bytes widened to halves (even and odd bytes apart): t + 0x100 - d has bit 8 set iff d <= t, and stays positive, so one
        // 32-bit subtraction serves both halves
        const uint32_t t2 = (t + 0x100u) * 0x00010001u;
        const uint32_t fe = ((t2 - absdiff(x & 0x00FF00FFu, y & 0x00FF00FFu)) >> 8) & 0x00010001u;
        const uint32_t fo = ((t2 - absdiff((x >> 8) & 0x00FF00FFu, (y >> 8) & 0x00FF00FFu)) >> 8) & 0x00010001u;
        return ((fe << 8) - fe) | (((fo << 8) - fo) << 8);
    } else {
        const uint32_t d = absdiff(x, y);
        return ((d & 0xFFFFu) <= t ? 0x0000FFFFu : 0u) | ((d >> 16) <= t ? 0xFFFF0000u : 0u);
    }
}

template <int ES, bool TEMPORAL> __device__ __forceinline__ uint32_t render_mix(uint32_t up, uint32_t dn, uint32_t ta, uint32_t tb, uint32_t t)
{
    const uint32_t spatial = render_avg<ES>(up, dn);
    if constexpr (!TEMPORAL) return spatial;
    const uint32_t m = render_within<ES>(ta, tb, t);
    return (render_avg<ES>(ta, tb) & m) | (spatial & ~m);
}

// one missing row: nb bytes at d from the rows up / dn (and ta / tb).  The vector form issues the 2 (4) loads of a lane's 16 bytes before
// their first use; the row's last nb % 16 bytes go container by container
template <int ES, bool VEC, bool TEMPORAL>
__device__ __forceinline__ void render_fill_row(uint8_t* d, const uint8_t* up, const uint8_t* dn, const uint8_t* ta, const uint8_t* tb, int nb, int t, int lane)
{
    typedef typename std::conditional<ES == 1, uint8_t, uint16_t>::type T;
    auto one = [&](int k) {                                                             // the container at byte k
        const int u = *reinterpret_cast<const T*>(up + k), w = *reinterpret_cast<const T*>(dn + k);
        int v = (u + w + 1) >> 1;
        if constexpr (TEMPORAL) {
            const int p = *reinterpret_cast<const T*>(ta + k), q = *reinterpret_cast<const T*>(tb + k);
            if ((p > q ? p - q : q - p) <= t) v = (p + q + 1) >> 1;
        }
        *reinterpret_cast<T*>(d + k) = (T)v;
    };
    if constexpr (VEC) {
        for (int x = lane * 16; x + 16 <= nb; x += 64 * 16) {
            const uint4 u = *reinterpret_cast<const uint4*>(up + x), w = *reinterpret_cast<const uint4*>(dn + x);
            uint4 p = u, q = u;
            if constexpr (TEMPORAL) { p = *reinterpret_cast<const uint4*>(ta + x); q = *reinterpret_cast<const uint4*>(tb + x); }
            uint4 o;
            o.x = render_mix<ES, TEMPORAL>(u.x, w.x, p.x, q.x, (uint32_t)t); o.y = render_mix<ES, TEMPORAL>(u.y, w.y, p.y, q.y, (uint32_t)t);
            o.z = render_mix<ES, TEMPORAL>(u.z, w.z, p.z, q.z, (uint32_t)t); o.w = render_mix<ES, TEMPORAL>(u.w, w.w, p.w, q.w, (uint32_t)t);
            *reinterpret_cast<uint4*>(d + x) = o;
        }
        for (int k = (nb & ~15) + lane * ES; k < nb; k += 64 * ES) one(k);             // the row's last nb % 16 bytes
    } else {
        for (int k = lane * ES; k < nb; k += 64 * ES) one(k);
    }
}

// VEC: every plane base, stride and pitch is a multiple of 16 bytes
template <int ES, bool VEC>
__global__ __launch_bounds__(256)
void kfm_render_kernel(RenderArgs a, const RenderEntry* __restrict__ plan, int row_blocks)
{
    const int frame = blockIdx.x / row_blocks, rb = blockIdx.x - frame * row_blocks;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const RenderEntry e = plan[frame];
    const int nrows = a.H + 2 * a.HUV;                                                  // Y rows, then U rows, then V rows
#pragma unroll 1
    for (int r = rb * kRenderRows + wave; r < min(nrows, (rb + 1) * kRenderRows); r += 4) {
        int pl, y;
        if (r < a.H) { pl = 0; y = r; } else if (r < a.H + a.HUV) { pl = 1; y = r - a.H; } else { pl = 2; y = r - a.H - a.HUV; }
        const uint8_t* sp = pl == 0 ? a.srcY : pl == 1 ? a.srcU : a.srcV;
        uint8_t* dp = pl == 0 ? a.dstY : pl == 1 ? a.dstU : a.dstV;
        const long long ss = pl == 0 ? a.src_strideY : a.src_strideUV, ds = pl == 0 ? a.dst_strideY : a.dst_strideUV;
        const int spitch = pl == 0 ? a.src_pitchY : a.src_pitchUV, dpitch = pl == 0 ? a.dst_pitchY : a.dst_pitchUV;
        const int nb = pl == 0 ? a.rowY : a.rowUV, h = pl == 0 ? a.H : a.HUV;
        auto srow = [&](int pic, int yy) { return sp + (long long)pic * ss + (long long)yy * spitch; };
        uint8_t* d = dp + (long long)frame * ds + (long long)y * dpitch;
        const int odd = y & 1;
        if (e.kind == 0 || odd == (e.kind == 2)) {
            // a woven or kept row: even rows from top, odd rows from bottom (the same picture for the bobs)
            const uint8_t* s = srow(odd ? e.bottom : e.top, y);
            if constexpr (VEC) {
                for (int x = lane * 16; x + 16 <= nb; x += 64 * 16) *reinterpret_cast<uint4*>(d + x) = *reinterpret_cast<const uint4*>(s + x);
                for (int k = (nb & ~15) + lane; k < nb; k += 64) d[k] = s[k];
            } else {
                for (int x = lane; x < nb; x += 64) d[x] = s[x];
            }
        } else {
            const int yu = y > 0 ? y - 1 : y + 1, yd = y + 1 < h ? y + 1 : y - 1;      // (h >= 2: one of the two neighbours always exists)
            const uint8_t *up = srow(e.top, yu), *dn = srow(e.top, yd);
            if (a.thresh >= 0) render_fill_row<ES, VEC, true>(d, up, dn, srow(e.top, y), srow(e.other, y), nb, a.thresh, lane);
            else render_fill_row<ES, VEC, false>(d, up, dn, nullptr, nullptr, nb, 0, lane);
        }
    }
}

hipError_t launch_kfm_render(hipStream_t st, const RenderArgs& a, const RenderEntry* dplan, int nout)
{
    if (nout <= 0) return hipSuccess;
    if (a.es != 1 && a.es != 2) return hipErrorInvalidValue;
    const int nrows = a.H + 2 * a.HUV;
    const long long row_blocks = (nrows + kRenderRows - 1) / kRenderRows;
    if (row_blocks * nout > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    dim3 grid((unsigned)(row_blocks * nout)), block(256);
    if (a.es == 1 && a.vec) hipLaunchKernelGGL((kfm_render_kernel<1, true>), grid, block, 0, st, a, dplan, (int)row_blocks);
    else if (a.es == 1) hipLaunchKernelGGL((kfm_render_kernel<1, false>), grid, block, 0, st, a, dplan, (int)row_blocks);
    else if (a.vec) hipLaunchKernelGGL((kfm_render_kernel<2, true>), grid, block, 0, st, a, dplan, (int)row_blocks);
    else hipLaunchKernelGGL((kfm_render_kernel<2, false>), grid, block, 0, st, a, dplan, (int)row_blocks);
    return hipGetLastError();
}

} // namespace amt
