// render_adaptive_kernels.hip -- the cadence renderer's edge-directed, motion-adaptive bob (self-specified, "parity unpinned"; DESIGN.md
// section 6d, "the adaptive rule").  WEAVE entries and the kept rows of a bob are moved exactly as kfm_render_kernel moves them; a missing
// row y of BOB_TOP(n) / BOB_BOTTOM(n) is, per pixel and in signed integers over the containers as stored,
//     U = C[y-1], D = C[y+1], c = U[x], e = D[x]                       (C = n, P = n - 1, N = n + 1; rows and columns clamped as below)
//     d = (A[y] + B[y]) >> 1                                            ((A, B) = (P, C) for BOB_TOP, (C, N) for BOB_BOTTOM)
//     diff = max(|A[y] - B[y]| >> 1, (|P[y-1] - c| + |P[y+1] - e|) >> 1, (|N[y-1] - c| + |N[y+1] - e|) >> 1)
//     pred = (U[x+j] + D[x-j]) >> 1 for the slope j of -2..2 with the smallest three-tap score sum |U[x+j+i] - D[x-j+i]|, i = -1..1 (j = 0
//            scores one less; -1 then -2, +1 then +2 against the running score, +-2 only where +-1 improved)
//     b = (A[y-2] + B[y-2]) >> 1, f = (A[y+2] + B[y+2]) >> 1
//     diff = max(diff, min(d - e, d - c, max(b - c, f - e)), -max(d - e, d - c, min(b - c, f - e)))
//     out = pred clamped into [d - diff, d + diff]
// A row y - 1 / y + 1 outside the plane takes the other one, a row y - 2 / y + 2 outside it takes y; a column outside it takes the nearest.
// One wave per output row, 16 bytes per lane where everything is 16-byte aligned: the 12 row segments of a lane's span are loaded
// before the first use, the three containers to the left and right of a span come from the neighbouring lanes' registers (v_mov_b32_dpp
// wave_shr:1 / wave_shl:1; no LDS), and only the lanes at the seams -- lane 0, lane 63, the row's last 16-byte span -- load theirs
// container by container with the column clamp.  8-bit containers are computed two to a register in 16-bit halves (every intermediate
// lies in [-765, 765]), 16-bit containers one to a register in 32 bits (differences need 17 bits and a sign).  No LDS, no atomics, no
// scratch.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "kernels.hpp"

namespace amt {

namespace {

constexpr int kAdpRows = 4;         // rows per workgroup (one wave per row)

typedef short adp_s2 __attribute__((ext_vector_type(2)));

struct AdpRow { const uint8_t* base; uint32_t off; };                                  // a row: base + off

// The 12 rows an interpolated row reads, as three pictures (C, P, N; A and B are two of them) at one row and five byte offsets from it: 15
// scalar registers where 12 pointers take 24
struct AdpRows {
    const uint8_t *c, *p, *n, *a, *b;                                                   // row max(y - 2, 0) of the pictures
    uint32_t o0, o1m, o1p, o2m, o2p;                                                    // rows y, y -+ 1, y -+ 2 (clamped) from there, in bytes
    __device__ __forceinline__ AdpRow u() const { return {c, o1m}; }
    __device__ __forceinline__ AdpRow d() const { return {c, o1p}; }
    __device__ __forceinline__ AdpRow pm() const { return {p, o1m}; }
    __device__ __forceinline__ AdpRow pp() const { return {p, o1p}; }
    __device__ __forceinline__ AdpRow nm() const { return {n, o1m}; }
    __device__ __forceinline__ AdpRow np() const { return {n, o1p}; }
    __device__ __forceinline__ AdpRow a0() const { return {a, o0}; }
    __device__ __forceinline__ AdpRow b0() const { return {b, o0}; }
    __device__ __forceinline__ AdpRow am() const { return {a, o2m}; }
    __device__ __forceinline__ AdpRow bm() const { return {b, o2m}; }
    __device__ __forceinline__ AdpRow ap() const { return {a, o2p}; }
    __device__ __forceinline__ AdpRow bp() const { return {b, o2p}; }
};

// v, with its origin hidden from the optimiser (no instruction).  Without it the compiler takes the packed form apart again: the sign
// mask becomes a compare and a select per 16-bit half, the unpacked bytes become byte-selecting 16-bit operations whose results are
// permuted back into pairs -- 1 550 vector instructions per 16-byte span against 1 200 with the halves kept together
__device__ __forceinline__ uint32_t adp_opaque(uint32_t v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ adp_s2 adp_opaque(adp_s2 v) { return __builtin_bit_cast(adp_s2, adp_opaque(__builtin_bit_cast(uint32_t, v))); }
__device__ __forceinline__ int adp_opaque(int v) { return v; }

// The rule on pixels held in V: int (one pixel) or adp_s2 (two pixels, 8-bit containers only).  u[j + 3] / w[j + 3]: U / D at column
// x + j.  SH: the sign bit of a lane of V.  Selects are bitwise under all-ones masks, so one text serves both
template <class V, class E, int SH>
__device__ __forceinline__ V adp_pixel(const V (&u)[7], const V (&w)[7], V pm, V pp, V nm, V np, V a0, V b0, V am, V bm, V ap, V bp)
{
    auto ad = [](V p, V q) { return __builtin_elementwise_abs(p - q); };
    auto mx2 = [](V p, V q) { return __builtin_elementwise_max(p, q); };
    auto mn2 = [](V p, V q) { return __builtin_elementwise_min(p, q); };
    auto sel = [](V m, V p, V q) { return (p & m) | (q & ~m); };
    const V c = u[3], e = w[3];
    const V d = (a0 + b0) >> (E)1;
    V diff = mx2(ad(a0, b0) >> (E)1, mx2((ad(pm, c) + ad(pp, e)) >> (E)1, (ad(nm, c) + ad(np, e)) >> (E)1));
    V pred = (c + e) >> (E)1;
    V score = ad(u[2], w[2]) + ad(c, e) + ad(u[4], w[4]) - (E)1;
#pragma unroll
    for (int sgn = -1; sgn <= 1; sgn += 2) {
        V alive = ~(V)(E)0;
#pragma unroll
        for (int m = 1; m <= 2; ++m) {
            const int j = sgn * m;
            const V s = ad(u[3 + j - 1], w[3 - j - 1]) + ad(u[3 + j], w[3 - j]) + ad(u[3 + j + 1], w[3 - j + 1]);
            const V take = adp_opaque(alive & ((s - score) >> (E)SH));                  // s < score (|s - score| <= 3 * the range: no overflow)
            score = sel(take, s, score);
            pred = sel(take, (u[3 + j] + w[3 - j]) >> (E)1, pred);
            alive = take;
        }
    }
    const V b = (am + bm) >> (E)1, f = (ap + bp) >> (E)1;
    const V mx = mx2(mx2(d - e, d - c), mn2(b - c, f - e)), mn = mn2(mn2(d - e, d - c), mx2(b - c, f - e));
    diff = mx2(mx2(diff, mn), -mx);
    return mx2(mn2(pred, d + diff), d - diff);                                           // diff >= 0: the band is never empty
}

// the container at column xi (clamped into the row of w containers)
template <int ES> __device__ __forceinline__ int adp_ld(AdpRow row, int xi, int w)
{
    typedef typename std::conditional<ES == 1, uint8_t, uint16_t>::type T;
    return *reinterpret_cast<const T*>(row.base + (row.off + (uint32_t)(min(max(xi, 0), w - 1) * ES)));
}

// one pixel, container by container
template <int ES> __device__ __forceinline__ void adp_one(uint8_t* d, const AdpRows& r, int xi, int w)
{
    typedef typename std::conditional<ES == 1, uint8_t, uint16_t>::type T;
    int u[7], dn[7];
#pragma unroll
    for (int j = -3; j <= 3; ++j) { u[j + 3] = adp_ld<ES>(r.u(), xi + j, w); dn[j + 3] = adp_ld<ES>(r.d(), xi + j, w); }
    auto at = [&](AdpRow row) { return (int)*reinterpret_cast<const T*>(row.base + (row.off + (uint32_t)(xi * ES))); };
    reinterpret_cast<T*>(d)[xi] = (T)adp_pixel<int, int, 31>(u, dn, at(r.pm()), at(r.pp()), at(r.nm()), at(r.np()), at(r.a0()), at(r.b0()), at(r.am()), at(r.bm()), at(r.ap()), at(r.bp()));
}

// lane i takes v of lane i - 1 / i + 1 (lane 0 / 63, and a lane whose source is inactive: 0)
__device__ __forceinline__ uint32_t adp_from_left(uint32_t v) { return __builtin_amdgcn_update_dpp(0u, v, 0x138, 0xF, 0xF, false); }     // wave_shr:1
__device__ __forceinline__ uint32_t adp_from_right(uint32_t v) { return __builtin_amdgcn_update_dpp(0u, v, 0x130, 0xF, 0xF, false); }    // wave_shl:1

// U or D of a 16-byte span with its three containers on either side.  8 bits: the dwords before, of and behind the span split into even and
// odd bytes in 16-bit halves (E, O: pixels 4k, 4k + 2 and 4k + 1, 4k + 3 of dword k) and the same moved on by two pixels (Eh, Oh), so
// that the pair of pixels (q, q + 2) is one register for every q
struct AdpSpan8 {
    adp_s2 E[6], O[6], Eh[5], Oh[5];
    __device__ __forceinline__ AdpSpan8(uint32_t l, uint4 v, uint32_t r)
    {
        const uint32_t x[6] = {l, v.x, v.y, v.z, v.w, r};
        uint32_t e[6], o[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) { e[k] = adp_opaque(x[k] & 0x00FF00FFu); o[k] = adp_opaque((x[k] >> 8) & 0x00FF00FFu); E[k] = __builtin_bit_cast(adp_s2, e[k]); O[k] = __builtin_bit_cast(adp_s2, o[k]); }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            Eh[k] = __builtin_bit_cast(adp_s2, __builtin_amdgcn_alignbit(e[k + 1], e[k], 16));
            Oh[k] = __builtin_bit_cast(adp_s2, __builtin_amdgcn_alignbit(o[k + 1], o[k], 16));
        }
    }
    // pixels (q, q + 2), q counted from the span's first pixel, -4 <= q <= 16
    __device__ __forceinline__ adp_s2 at(int q) const
    {
        const int k = (q + 4) >> 2, r = (q + 4) & 3;
        return r == 0 ? E[k] : r == 1 ? O[k] : r == 2 ? Eh[k] : Oh[k];
    }
};

template <int ES, bool VEC>
__device__ __forceinline__ void adp_fill_row(uint8_t* d, const AdpRows& r, int nb, int lane)
{
    const int w = nb / ES;
    if constexpr (!VEC) {
        for (int xi = lane; xi < w; xi += 64) adp_one<ES>(d, r, xi, w);
        return;
    } else {
        for (int x = lane * 16; x + 16 <= nb; x += 64 * 16) {
            auto ld = [&](AdpRow row) { return *reinterpret_cast<const uint4*>(row.base + (row.off + (uint32_t)x)); };
            const uint4 u = ld(r.u()), dn = ld(r.d()), pm = ld(r.pm()), pp = ld(r.pp()), nm = ld(r.nm()), np = ld(r.np());
            const uint4 a0 = ld(r.a0()), b0 = ld(r.b0()), am = ld(r.am()), bm = ld(r.bm()), ap = ld(r.ap()), bp = ld(r.bp());
            const int xi = x / ES;                                                      // the span's first column
            const bool first = lane == 0, last = lane == 63 || x + 32 > nb;            // no lane with the left / right neighbours in its registers
            uint4 o;
            if constexpr (ES == 1) {
                uint32_t ul = adp_from_left(u.w), ur = adp_from_right(u.x), dl = adp_from_left(dn.w), dr = adp_from_right(dn.x);
                if (first) {
                    ul = (uint32_t)adp_ld<1>(r.u(), xi - 3, w) << 8 | (uint32_t)adp_ld<1>(r.u(), xi - 2, w) << 16 | (uint32_t)adp_ld<1>(r.u(), xi - 1, w) << 24;
                    dl = (uint32_t)adp_ld<1>(r.d(), xi - 3, w) << 8 | (uint32_t)adp_ld<1>(r.d(), xi - 2, w) << 16 | (uint32_t)adp_ld<1>(r.d(), xi - 1, w) << 24;
                }
                if (last) {
                    ur = (uint32_t)adp_ld<1>(r.u(), xi + 16, w) | (uint32_t)adp_ld<1>(r.u(), xi + 17, w) << 8 | (uint32_t)adp_ld<1>(r.u(), xi + 18, w) << 16;
                    dr = (uint32_t)adp_ld<1>(r.d(), xi + 16, w) | (uint32_t)adp_ld<1>(r.d(), xi + 17, w) << 8 | (uint32_t)adp_ld<1>(r.d(), xi + 18, w) << 16;
                }
                const AdpSpan8 U(ul, u, ur), D(dl, dn, dr);
                const uint32_t PM[4] = {pm.x, pm.y, pm.z, pm.w}, PP[4] = {pp.x, pp.y, pp.z, pp.w}, NM[4] = {nm.x, nm.y, nm.z, nm.w}, NP[4] = {np.x, np.y, np.z, np.w};
                const uint32_t A0[4] = {a0.x, a0.y, a0.z, a0.w}, B0[4] = {b0.x, b0.y, b0.z, b0.w}, AM[4] = {am.x, am.y, am.z, am.w}, BM[4] = {bm.x, bm.y, bm.z, bm.w};
                const uint32_t AP[4] = {ap.x, ap.y, ap.z, ap.w}, BP[4] = {bp.x, bp.y, bp.z, bp.w};
                uint32_t O[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint32_t res[2];
#pragma unroll
                    for (int par = 0; par < 2; ++par) {                                 // pixels 4k + par and 4k + par + 2
                        auto half = [&](uint32_t v) { return __builtin_bit_cast(adp_s2, adp_opaque((v >> (8 * par)) & 0x00FF00FFu)); };
                        adp_s2 uu[7], ww[7];
#pragma unroll
                        for (int j = -3; j <= 3; ++j) { uu[j + 3] = U.at(4 * k + par + j); ww[j + 3] = D.at(4 * k + par + j); }
                        res[par] = __builtin_bit_cast(uint32_t, adp_pixel<adp_s2, short, 15>(uu, ww, half(PM[k]), half(PP[k]), half(NM[k]), half(NP[k]), half(A0[k]), half(B0[k]),
                                                                                                 half(AM[k]), half(BM[k]), half(AP[k]), half(BP[k])));
                    }
                    O[k] = res[0] | res[1] << 8;                                        // every result lies in 0..255
                }
                o = uint4{O[0], O[1], O[2], O[3]};
            } else {
                uint32_t ul0 = adp_from_left(u.z), ul1 = adp_from_left(u.w), ur0 = adp_from_right(u.x), ur1 = adp_from_right(u.y);
                uint32_t dl0 = adp_from_left(dn.z), dl1 = adp_from_left(dn.w), dr0 = adp_from_right(dn.x), dr1 = adp_from_right(dn.y);
                if (first) {
                    ul0 = (uint32_t)adp_ld<2>(r.u(), xi - 3, w) << 16; ul1 = (uint32_t)adp_ld<2>(r.u(), xi - 2, w) | (uint32_t)adp_ld<2>(r.u(), xi - 1, w) << 16;
                    dl0 = (uint32_t)adp_ld<2>(r.d(), xi - 3, w) << 16; dl1 = (uint32_t)adp_ld<2>(r.d(), xi - 2, w) | (uint32_t)adp_ld<2>(r.d(), xi - 1, w) << 16;
                }
                if (last) {
                    ur0 = (uint32_t)adp_ld<2>(r.u(), xi + 8, w) | (uint32_t)adp_ld<2>(r.u(), xi + 9, w) << 16; ur1 = (uint32_t)adp_ld<2>(r.u(), xi + 10, w);
                    dr0 = (uint32_t)adp_ld<2>(r.d(), xi + 8, w) | (uint32_t)adp_ld<2>(r.d(), xi + 9, w) << 16; dr1 = (uint32_t)adp_ld<2>(r.d(), xi + 10, w);
                }
                const uint32_t UX[8] = {ul0, ul1, u.x, u.y, u.z, u.w, ur0, ur1}, DX[8] = {dl0, dl1, dn.x, dn.y, dn.z, dn.w, dr0, dr1};
                const uint32_t PM[4] = {pm.x, pm.y, pm.z, pm.w}, PP[4] = {pp.x, pp.y, pp.z, pp.w}, NM[4] = {nm.x, nm.y, nm.z, nm.w}, NP[4] = {np.x, np.y, np.z, np.w};
                const uint32_t A0[4] = {a0.x, a0.y, a0.z, a0.w}, B0[4] = {b0.x, b0.y, b0.z, b0.w}, AM[4] = {am.x, am.y, am.z, am.w}, BM[4] = {bm.x, bm.y, bm.z, bm.w};
                const uint32_t AP[4] = {ap.x, ap.y, ap.z, ap.w}, BP[4] = {bp.x, bp.y, bp.z, bp.w};
                auto px = [](const uint32_t* v, int q) { return (int)((v[q >> 1] >> (16 * (q & 1))) & 0xFFFFu); };      // container q of the dwords v
                uint32_t O[4] = {0, 0, 0, 0};
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    int uu[7], ww[7];
#pragma unroll
                    for (int j = -3; j <= 3; ++j) { uu[j + 3] = px(UX, g + j + 4); ww[j + 3] = px(DX, g + j + 4); }
                    const int v = adp_pixel<int, int, 31>(uu, ww, px(PM, g), px(PP, g), px(NM, g), px(NP, g), px(A0, g), px(B0, g), px(AM, g), px(BM, g), px(AP, g), px(BP, g));
                    O[g >> 1] |= (uint32_t)v << (16 * (g & 1));                        // every result lies in 0..65535
                }
                o = uint4{O[0], O[1], O[2], O[3]};
            }
            *reinterpret_cast<uint4*>(d + x) = o;
        }
        for (int xi = (nb & ~15) / ES + lane; xi < w; xi += 64) adp_one<ES>(d, r, xi, w);                                // the row's last nb % 16 bytes
    }
}

} // namespace

// VEC: every plane base, stride and pitch is a multiple of 16 bytes
template <int ES, bool VEC>
__global__ __launch_bounds__(256)
void kfm_render_adaptive_kernel(RenderArgs a, const RenderAdaptiveEntry* __restrict__ plan, int row_blocks)
{
    const int frame = blockIdx.x / row_blocks, rb = blockIdx.x - frame * row_blocks;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const RenderAdaptiveEntry e = plan[frame];
    const int nrows = a.H + 2 * a.HUV;                                                  // Y rows, then U rows, then V rows
    const int r = rb * kAdpRows + wave;                                                  // one row per wave, no loop: nothing but the row stays live
    if (r < nrows) {
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
            // (h >= 2: one of the rows y - 1, y + 1 always exists)
            const int y1m = y > 0 ? y - 1 : y + 1, y1p = y + 1 < h ? y + 1 : y - 1, y2m = y >= 2 ? y - 2 : y, y2p = y + 2 < h ? y + 2 : y;
            const int pa = e.kind == 1 ? e.prev : e.top, pb = e.kind == 1 ? e.top : e.next;   // the missing parity's fields before and after the kept one
            const int y0 = max(y - 2, 0);                                               // every row read lies in [y0, y0 + 4]
            auto off = [&](int yy) { return (uint32_t)((yy - y0) * spitch); };
            const AdpRows rows = {srow(e.top, y0), srow(e.prev, y0), srow(e.next, y0), srow(pa, y0), srow(pb, y0), off(y), off(y1m), off(y1p), off(y2m), off(y2p)};
            adp_fill_row<ES, VEC>(d, rows, nb, lane);
        }
    }
}

hipError_t launch_kfm_render_adaptive(hipStream_t st, const RenderArgs& a, const RenderAdaptiveEntry* dplan, int nout)
{
    if (nout <= 0) return hipSuccess;
    if (a.es != 1 && a.es != 2) return hipErrorInvalidValue;
    const int nrows = a.H + 2 * a.HUV;
    const long long row_blocks = (nrows + kAdpRows - 1) / kAdpRows;
    if (row_blocks * nout > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    dim3 grid((unsigned)(row_blocks * nout)), block(256);
    if (a.es == 1 && a.vec) hipLaunchKernelGGL((kfm_render_adaptive_kernel<1, true>), grid, block, 0, st, a, dplan, (int)row_blocks);
    else if (a.es == 1) hipLaunchKernelGGL((kfm_render_adaptive_kernel<1, false>), grid, block, 0, st, a, dplan, (int)row_blocks);
    else if (a.vec) hipLaunchKernelGGL((kfm_render_adaptive_kernel<2, true>), grid, block, 0, st, a, dplan, (int)row_blocks);
    else hipLaunchKernelGGL((kfm_render_adaptive_kernel<2, false>), grid, block, 0, st, a, dplan, (int)row_blocks);
    return hipGetLastError();
}

} // namespace amt
