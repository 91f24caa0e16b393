// render_adaptive_body.h -- the text of the adaptive rule ("the adaptive rule") that the planar kernels
// (render_adaptive_kernels.hip) and the decoder-surface kernels (render_adaptive_surface_kernels.hip) share: the rule on one or two
// pixels (adp_pixel), the opaque helpers that keep the packed form together, the row bundle, the DPP wave shifts, the packed span of an
// 8-bit row, and the row function itself.  The row function has two template arguments the planar kernels leave at their defaults:
//   MSB   samples are containers >> s: one v_pk_lshrrev_b16 per loaded dword (and per dword of the neighbouring lanes) before any
//         arithmetic, one v_pk_lshlrev_b16 per stored dword, so a result has zero low bits.  16-bit containers only.  (Shifting each
//         container where it is taken out of its dword -- v_bfe_u32 / v_lshrrev_b32 by 16 + s -- issues no fewer instructions, because
//         the LSB form takes its halves out with SDWA operands for nothing, and held 116 to 124 VGPRs where this holds 84 to 104.)
//   STEP  1: the row is one plane.  2: the row is an interleaved UV row: neighbour j of container q is container q + 2j, and a column
//         outside the plane takes the nearest of ITS component: 2 * clamp((q >> 1) + j, 0, w / 2 - 1) + (q & 1).  A 16-byte span starts
//         on an even container, so the parity of a container within a span is its component.  A span needs six containers on either
//         side of U and D: two dwords of the neighbouring lane at 8 bits, three at 16.
// With <MSB = false, STEP = 1> every function below is the text the planar kernels had in their own file, and they compile to the same
// instruction streams as before.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "pack16.h"

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

// the container at column xi (clamped into the row of w containers; STEP 2: clamped within its component of an interleaved row)
template <int ES, int STEP = 1> __device__ __forceinline__ int adp_ld(AdpRow row, int xi, int w)
{
    typedef typename std::conditional<ES == 1, uint8_t, uint16_t>::type T;
    if constexpr (STEP == 1) return *reinterpret_cast<const T*>(row.base + (row.off + (uint32_t)(min(max(xi, 0), w - 1) * ES)));
    else return *reinterpret_cast<const T*>(row.base + (row.off + (uint32_t)((2 * min(max(xi >> 1, 0), (w >> 1) - 1) + (xi & 1)) * ES)));
}

// one pixel, container by container
template <int ES, bool MSB = false, int STEP = 1> __device__ __forceinline__ void adp_one(uint8_t* d, const AdpRows& r, int xi, int w, int s = 0)
{
    typedef typename std::conditional<ES == 1, uint8_t, uint16_t>::type T;
    static_assert(!MSB || ES == 2, "MSB-aligned containers are 16-bit ones");
    int u[7], dn[7];
#pragma unroll
    for (int j = -3; j <= 3; ++j) { u[j + 3] = adp_ld<ES, STEP>(r.u(), xi + STEP * j, w); dn[j + 3] = adp_ld<ES, STEP>(r.d(), xi + STEP * j, w); }
    auto at = [&](AdpRow row) { return (int)*reinterpret_cast<const T*>(row.base + (row.off + (uint32_t)(xi * ES))); };
    if constexpr (!MSB) {
        reinterpret_cast<T*>(d)[xi] = (T)adp_pixel<int, int, 31>(u, dn, at(r.pm()), at(r.pp()), at(r.nm()), at(r.np()), at(r.a0()), at(r.b0()), at(r.am()), at(r.bm()), at(r.ap()), at(r.bp()));
    } else {
#pragma unroll
        for (int j = 0; j < 7; ++j) { u[j] >>= s; dn[j] >>= s; }
        auto sm = [&](AdpRow row) { return at(row) >> s; };
        reinterpret_cast<T*>(d)[xi] = (T)(adp_pixel<int, int, 31>(u, dn, sm(r.pm()), sm(r.pp()), sm(r.nm()), sm(r.np()), sm(r.a0()), sm(r.b0()), sm(r.am()), sm(r.bm()), sm(r.ap()), sm(r.bp())) << s);
    }
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
    // the byte half par of dword k (pixels 4k + par and 4k + par + 2), moved on by j columns
    __device__ __forceinline__ adp_s2 pair(int k, int par, int j) const { return at(4 * k + par + j); }
    static __device__ __forceinline__ AdpSpan8 of(uint32_t, uint32_t l, uint4 v, uint32_t r, uint32_t) { return AdpSpan8(l, v, r); }
};

// The same of an interleaved UV row: the pair (q, q + 2) is two neighbouring samples of ONE component, so the even bytes are U, U and the
// odd ones V, V, and a step of one column is a step of two containers: E, O hold the components (2k, 2k + 1) of dword k, Eh, Oh the
// components (2k + 1, 2k + 2).  Three columns on either side are six containers: two dwords before and two behind the span
struct AdpSpan8UV {
    adp_s2 E[8], O[8], Eh[7], Oh[7];
    __device__ __forceinline__ AdpSpan8UV(uint32_t l0, uint32_t l1, uint4 v, uint32_t r0, uint32_t r1)
    {
        const uint32_t x[8] = {l0, l1, v.x, v.y, v.z, v.w, r0, r1};
        uint32_t e[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { e[k] = adp_opaque(x[k] & 0x00FF00FFu); o[k] = adp_opaque((x[k] >> 8) & 0x00FF00FFu); E[k] = __builtin_bit_cast(adp_s2, e[k]); O[k] = __builtin_bit_cast(adp_s2, o[k]); }
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            Eh[k] = __builtin_bit_cast(adp_s2, __builtin_amdgcn_alignbit(e[k + 1], e[k], 16));
            Oh[k] = __builtin_bit_cast(adp_s2, __builtin_amdgcn_alignbit(o[k + 1], o[k], 16));
        }
    }
    // columns (m, m + 1) of component par (0: U, 1: V), m counted from the span's first column, -3 <= m <= 9
    __device__ __forceinline__ adp_s2 at(int m, int par) const
    {
        const int k = (m + 4) >> 1;
        return (m + 4) & 1 ? (par ? Oh[k] : Eh[k]) : (par ? O[k] : E[k]);
    }
    // the byte half par of dword k (columns 2k and 2k + 1 of component par), moved on by j columns
    __device__ __forceinline__ adp_s2 pair(int k, int par, int j) const { return at(2 * k + j, par); }
    static __device__ __forceinline__ AdpSpan8UV of(uint32_t l0, uint32_t l1, uint4 v, uint32_t r0, uint32_t r1) { return AdpSpan8UV(l0, l1, v, r0, r1); }
};

template <int ES, bool VEC, bool MSB = false, int STEP = 1>
__device__ __forceinline__ void adp_fill_row(uint8_t* d, const AdpRows& r, int nb, int lane, int s = 0)
{
    static_assert(!MSB || ES == 2, "MSB-aligned containers are 16-bit ones");
    const int w = nb / ES;
    if constexpr (!VEC) {
        for (int xi = lane; xi < w; xi += 64) adp_one<ES, MSB, STEP>(d, r, xi, w, s);
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
                typedef typename std::conditional<STEP == 1, AdpSpan8, AdpSpan8UV>::type Span;
                uint32_t ul = adp_from_left(u.w), ur = adp_from_right(u.x), dl = adp_from_left(dn.w), dr = adp_from_right(dn.x);
                uint32_t ul0 = 0, ur1 = 0, dl0 = 0, dr1 = 0;                           // STEP 2: the dwords one further out
                if constexpr (STEP == 2) { ul0 = adp_from_left(u.z); ur1 = adp_from_right(u.y); dl0 = adp_from_left(dn.z); dr1 = adp_from_right(dn.y); }
                if (first) {
                    if constexpr (STEP == 1) {
                        ul = (uint32_t)adp_ld<1>(r.u(), xi - 3, w) << 8 | (uint32_t)adp_ld<1>(r.u(), xi - 2, w) << 16 | (uint32_t)adp_ld<1>(r.u(), xi - 1, w) << 24;
                        dl = (uint32_t)adp_ld<1>(r.d(), xi - 3, w) << 8 | (uint32_t)adp_ld<1>(r.d(), xi - 2, w) << 16 | (uint32_t)adp_ld<1>(r.d(), xi - 1, w) << 24;
                    } else {
                        // columns -3..-1 of both components: containers xi - 6 .. xi - 1
                        ul0 = (uint32_t)adp_ld<1, 2>(r.u(), xi - 6, w) << 16 | (uint32_t)adp_ld<1, 2>(r.u(), xi - 5, w) << 24;
                        dl0 = (uint32_t)adp_ld<1, 2>(r.d(), xi - 6, w) << 16 | (uint32_t)adp_ld<1, 2>(r.d(), xi - 5, w) << 24;
                        ul = (uint32_t)adp_ld<1, 2>(r.u(), xi - 4, w) | (uint32_t)adp_ld<1, 2>(r.u(), xi - 3, w) << 8 | (uint32_t)adp_ld<1, 2>(r.u(), xi - 2, w) << 16 | (uint32_t)adp_ld<1, 2>(r.u(), xi - 1, w) << 24;
                        dl = (uint32_t)adp_ld<1, 2>(r.d(), xi - 4, w) | (uint32_t)adp_ld<1, 2>(r.d(), xi - 3, w) << 8 | (uint32_t)adp_ld<1, 2>(r.d(), xi - 2, w) << 16 | (uint32_t)adp_ld<1, 2>(r.d(), xi - 1, w) << 24;
                    }
                }
                if (last) {
                    if constexpr (STEP == 1) {
                        ur = (uint32_t)adp_ld<1>(r.u(), xi + 16, w) | (uint32_t)adp_ld<1>(r.u(), xi + 17, w) << 8 | (uint32_t)adp_ld<1>(r.u(), xi + 18, w) << 16;
                        dr = (uint32_t)adp_ld<1>(r.d(), xi + 16, w) | (uint32_t)adp_ld<1>(r.d(), xi + 17, w) << 8 | (uint32_t)adp_ld<1>(r.d(), xi + 18, w) << 16;
                    } else {
                        // columns 8..10 of both components: containers xi + 16 .. xi + 21
                        ur = (uint32_t)adp_ld<1, 2>(r.u(), xi + 16, w) | (uint32_t)adp_ld<1, 2>(r.u(), xi + 17, w) << 8 | (uint32_t)adp_ld<1, 2>(r.u(), xi + 18, w) << 16 | (uint32_t)adp_ld<1, 2>(r.u(), xi + 19, w) << 24;
                        dr = (uint32_t)adp_ld<1, 2>(r.d(), xi + 16, w) | (uint32_t)adp_ld<1, 2>(r.d(), xi + 17, w) << 8 | (uint32_t)adp_ld<1, 2>(r.d(), xi + 18, w) << 16 | (uint32_t)adp_ld<1, 2>(r.d(), xi + 19, w) << 24;
                        ur1 = (uint32_t)adp_ld<1, 2>(r.u(), xi + 20, w) | (uint32_t)adp_ld<1, 2>(r.u(), xi + 21, w) << 8;
                        dr1 = (uint32_t)adp_ld<1, 2>(r.d(), xi + 20, w) | (uint32_t)adp_ld<1, 2>(r.d(), xi + 21, w) << 8;
                    }
                }
                const Span U = Span::of(ul0, ul, u, ur, ur1), D = Span::of(dl0, dl, dn, dr, dr1);
                const uint32_t PM[4] = {pm.x, pm.y, pm.z, pm.w}, PP[4] = {pp.x, pp.y, pp.z, pp.w}, NM[4] = {nm.x, nm.y, nm.z, nm.w}, NP[4] = {np.x, np.y, np.z, np.w};
                const uint32_t A0[4] = {a0.x, a0.y, a0.z, a0.w}, B0[4] = {b0.x, b0.y, b0.z, b0.w}, AM[4] = {am.x, am.y, am.z, am.w}, BM[4] = {bm.x, bm.y, bm.z, bm.w};
                const uint32_t AP[4] = {ap.x, ap.y, ap.z, ap.w}, BP[4] = {bp.x, bp.y, bp.z, bp.w};
                uint32_t O[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint32_t res[2];
#pragma unroll
                    for (int par = 0; par < 2; ++par) {                                 // the even bytes of dword k, then the odd ones: two pixels of one plane
                        auto half = [&](uint32_t v) { return __builtin_bit_cast(adp_s2, adp_opaque((v >> (8 * par)) & 0x00FF00FFu)); };
                        adp_s2 uu[7], ww[7];
#pragma unroll
                        for (int j = -3; j <= 3; ++j) { uu[j + 3] = U.pair(k, par, j); ww[j + 3] = D.pair(k, par, j); }
                        res[par] = __builtin_bit_cast(uint32_t, adp_pixel<adp_s2, short, 15>(uu, ww, half(PM[k]), half(PP[k]), half(NM[k]), half(NP[k]), half(A0[k]), half(B0[k]),
                                                                                                 half(AM[k]), half(BM[k]), half(AP[k]), half(BP[k])));
                    }
                    O[k] = res[0] | res[1] << 8;                                        // every result lies in 0..255
                }
                o = uint4{O[0], O[1], O[2], O[3]};
            } else {
                constexpr int NL = STEP == 1 ? 2 : 3;                                   // dwords of the neighbouring lane on either side: 3 (6) containers
                uint32_t UX[4 + 2 * NL], DX[4 + 2 * NL];
                if constexpr (STEP == 1) {
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
                    const uint32_t ux[8] = {ul0, ul1, u.x, u.y, u.z, u.w, ur0, ur1}, dx[8] = {dl0, dl1, dn.x, dn.y, dn.z, dn.w, dr0, dr1};
#pragma unroll
                    for (int k = 0; k < 8; ++k) { UX[k] = ux[k]; DX[k] = dx[k]; }
                } else {
                    // columns -3..-1 and 4..6 of both components: containers xi - 6 .. xi - 1 and xi + 8 .. xi + 13
                    uint32_t ul[3] = {adp_from_left(u.y), adp_from_left(u.z), adp_from_left(u.w)}, ur[3] = {adp_from_right(u.x), adp_from_right(u.y), adp_from_right(u.z)};
                    uint32_t dl[3] = {adp_from_left(dn.y), adp_from_left(dn.z), adp_from_left(dn.w)}, dr[3] = {adp_from_right(dn.x), adp_from_right(dn.y), adp_from_right(dn.z)};
                    auto two = [&](AdpRow row, int q) { return (uint32_t)adp_ld<2, 2>(row, q, w) | (uint32_t)adp_ld<2, 2>(row, q + 1, w) << 16; };
                    if (first) {
#pragma unroll
                        for (int t = 0; t < 3; ++t) { ul[t] = two(r.u(), xi - 6 + 2 * t); dl[t] = two(r.d(), xi - 6 + 2 * t); }
                    }
                    if (last) {
#pragma unroll
                        for (int t = 0; t < 3; ++t) { ur[t] = two(r.u(), xi + 8 + 2 * t); dr[t] = two(r.d(), xi + 8 + 2 * t); }
                    }
                    const uint32_t ux[10] = {ul[0], ul[1], ul[2], u.x, u.y, u.z, u.w, ur[0], ur[1], ur[2]}, dx[10] = {dl[0], dl[1], dl[2], dn.x, dn.y, dn.z, dn.w, dr[0], dr[1], dr[2]};
#pragma unroll
                    for (int k = 0; k < 10; ++k) { UX[k] = ux[k]; DX[k] = dx[k]; }
                }
                uint32_t PM[4] = {pm.x, pm.y, pm.z, pm.w}, PP[4] = {pp.x, pp.y, pp.z, pp.w}, NM[4] = {nm.x, nm.y, nm.z, nm.w}, NP[4] = {np.x, np.y, np.z, np.w};
                uint32_t A0[4] = {a0.x, a0.y, a0.z, a0.w}, B0[4] = {b0.x, b0.y, b0.z, b0.w}, AM[4] = {am.x, am.y, am.z, am.w}, BM[4] = {bm.x, bm.y, bm.z, bm.w};
                uint32_t AP[4] = {ap.x, ap.y, ap.z, ap.w}, BP[4] = {bp.x, bp.y, bp.z, bp.w};
                if constexpr (MSB) {
                    // containers to samples, both halves of a dword at once, before any arithmetic
#pragma unroll
                    for (int k = 0; k < 4 + 2 * NL; ++k) { UX[k] = pk_shr16(UX[k], s); DX[k] = pk_shr16(DX[k], s); }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        PM[k] = pk_shr16(PM[k], s); PP[k] = pk_shr16(PP[k], s); NM[k] = pk_shr16(NM[k], s); NP[k] = pk_shr16(NP[k], s); A0[k] = pk_shr16(A0[k], s);
                        B0[k] = pk_shr16(B0[k], s); AM[k] = pk_shr16(AM[k], s); BM[k] = pk_shr16(BM[k], s); AP[k] = pk_shr16(AP[k], s); BP[k] = pk_shr16(BP[k], s);
                    }
                }
                auto px = [](const uint32_t* v, int q) { return (int)((v[q >> 1] >> (16 * (q & 1))) & 0xFFFFu); };      // container q of the dwords v
                uint32_t O[4] = {0, 0, 0, 0};
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    int uu[7], ww[7];
#pragma unroll
                    for (int j = -3; j <= 3; ++j) { uu[j + 3] = px(UX, g + STEP * j + 2 * NL); ww[j + 3] = px(DX, g + STEP * j + 2 * NL); }
                    const int v = adp_pixel<int, int, 31>(uu, ww, px(PM, g), px(PP, g), px(NM, g), px(NP, g), px(A0, g), px(B0, g), px(AM, g), px(BM, g), px(AP, g), px(BP, g));
                    O[g >> 1] |= (uint32_t)v << (16 * (g & 1));                        // every result lies in 0..65535
                }
                if constexpr (MSB) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) O[k] = pk_shl16(O[k], s);                // samples to containers, low bits zero
                }
                o = uint4{O[0], O[1], O[2], O[3]};
            }
            *reinterpret_cast<uint4*>(d + x) = o;
        }
        for (int xi = (nb & ~15) / ES + lane; xi < w; xi += 64) adp_one<ES, MSB, STEP>(d, r, xi, w, s);                 // the row's last nb % 16 bytes
    }
}

} // namespace

} // namespace amt
