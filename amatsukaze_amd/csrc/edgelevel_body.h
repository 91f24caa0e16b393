// edgelevel_body.h -- the text of the edge level's rule that edgelevel_kernels.hip (planar LSB planes) compiles and
// that kernels for decoder surfaces in kind can compile too: the rule on one or two pixels (edge_pixel), the ranks of nine, and the cell
// that filters a lane's 16 bytes of an output row out of a window of five rows held in registers.  A row of the window is six dwords:
// the lane's 16 bytes and the dword before and behind them, of which the rule reads two containers each.
//   8-bit containers are computed two to a register in 16-bit halves: the pair (q, q + 2) of a row is one register for every q (E, O:
//   the even and odd bytes of a dword; Eh, Oh: the same moved on by two pixels), every intermediate of the rule but the product lies in
//   [-4064, 4319] (T, at most 32767, is only subtracted from), and the product (c - avg) * strength, below 2^16 in magnitude, is
//   formed per pixel in 32 bits and packed again.
//   16-bit containers are one to a register in 32 bits.
// Selects are bitwise under all-ones masks taken from sign bits, so one text serves both.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

namespace amt {

namespace {

typedef short edge_s2 __attribute__((ext_vector_type(2)));

// v, with its origin hidden from the optimiser (no instruction): keeps the packed form together (render_adaptive_body.h, adp_opaque)
__device__ __forceinline__ uint32_t edge_opaque(uint32_t v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ edge_s2 edge_opaque(edge_s2 v) { return __builtin_bit_cast(edge_s2, edge_opaque(__builtin_bit_cast(uint32_t, v))); }
__device__ __forceinline__ int edge_opaque(int v) { return v; }

// ((c - avg) * strength) >> 4, the shift arithmetic: |c - avg| <= 32768 and strength <= 255, a signed 24-bit multiply
__device__ __forceinline__ int edge_scale(int d, int strength) { return __mul24(d, strength) >> 4; }
// (the instruction by name: of a product whose bits 4..19 alone are kept, the compiler forms the low half at full width)
__device__ __forceinline__ int edge_mul24(int a, int b)
{
    int r;
    asm("v_mul_i32_i24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ edge_s2 edge_scale(edge_s2 d, int strength)
{
    return edge_s2{(short)(edge_mul24((int)d.x, strength) >> 4), (short)(edge_mul24((int)d.y, strength) >> 4)};
}

// the middle of three
__device__ __forceinline__ int edge_med3(int a, int b, int c)
{
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ edge_s2 edge_med3(edge_s2 a, edge_s2 b, edge_s2 c)
{
    return __builtin_elementwise_max(__builtin_elementwise_min(a, b), __builtin_elementwise_min(__builtin_elementwise_max(a, b), c));
}

template <class V> struct EdgeLanes;
template <> struct EdgeLanes<int> { typedef int E; static constexpr int SH = 31; static __device__ __forceinline__ int splat(int v) { return v; } };
template <> struct EdgeLanes<edge_s2> { typedef short E; static constexpr int SH = 15; static __device__ __forceinline__ edge_s2 splat(int v) { return edge_s2{(short)v, (short)v}; } };

// The rule on pixels held in V: int (one pixel) or edge_s2 (two pixels, 8-bit containers only).  h[j]: s[y][x - 2 + j]; v[j]: s[y - 2 + j][x];
// u[j] / d[j]: s[y - 1][x - 1 + j] / s[y + 1][x - 1 + j].  REP: repair, 0..4.  The pixel is an interior one: the caller keeps the border's
template <class V, int REP>
__device__ __forceinline__ V edge_pixel(const V (&h)[5], const V (&v)[5], const V (&u)[3], const V (&d)[3], V thr, int strength)
{
    typedef typename EdgeLanes<V>::E E;
    constexpr int SH = EdgeLanes<V>::SH;
    auto mx2 = [](V p, V q) { return __builtin_elementwise_max(p, q); };
    auto mn2 = [](V p, V q) { return __builtin_elementwise_min(p, q); };
    auto ad = [](V p, V q) { return __builtin_elementwise_abs(p - q); };
    auto sel = [](V m, V p, V q) { return (p & m) | (q & ~m); };
    const V c = h[2];
    // direction: the line of the larger range, a tie the horizontal one
    const V hmx = mx2(mx2(mx2(h[0], h[1]), mx2(h[3], h[4])), c), hmn = mn2(mn2(mn2(h[0], h[1]), mn2(h[3], h[4])), c);
    const V vmx = mx2(mx2(mx2(v[0], v[1]), mx2(v[3], v[4])), c), vmn = mn2(mn2(mn2(v[0], v[1]), mn2(v[3], v[4])), c);
    const V vert = edge_opaque(((hmx - hmn) - (vmx - vmn)) >> (E)SH);                   // rh < rv
    const V l0 = sel(vert, v[0], h[0]), l1 = sel(vert, v[1], h[1]), l3 = sel(vert, v[3], h[3]), l4 = sel(vert, v[4], h[4]);
    const V mx = sel(vert, vmx, hmx), mn = sel(vert, vmn, hmn), rng = mx - mn;
    const V step = mx2(mx2(ad(l1, l0), ad(c, l1)), mx2(ad(l3, c), ad(l4, l3)));
    // levelled: rng > T, 4 step < 3 rng, 8 step > 3 rng -- three differences that are all negative
    const V three = rng + rng + rng;
    const V lev = edge_opaque(((thr - rng) & ((step << (E)2) - three) & (three - (step << (E)3))) >> (E)SH);
    const V avg = (mx + mn) >> (E)1;
    V e = mx2(mn2(c + edge_scale(c - avg, strength), mx), mn);
    if constexpr (REP > 0) {
        // the ranks n[REP - 1] and n[9 - REP] of the 3 x 3 around the pixel: each column sorted, then the rows of lows, middles and highs;
        // an entry of that table has at least (row + 1) * (column + 1) - 1 entries below it, which leaves few candidates for a rank
        V lo[3], mi[3], hi[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const V p = u[k], q = h[k + 1], r = d[k];
            lo[k] = mn2(mn2(p, q), r); hi[k] = mx2(mx2(p, q), r); mi[k] = edge_med3(p, q, r);
        }
        auto min3 = [&](const V (&t)[3]) { return mn2(mn2(t[0], t[1]), t[2]); };
        auto max3 = [&](const V (&t)[3]) { return mx2(mx2(t[0], t[1]), t[2]); };
        auto med3 = [&](const V (&t)[3]) { return edge_med3(t[0], t[1], t[2]); };
        V below, above;
        if constexpr (REP == 1) { below = min3(lo); above = max3(hi); }
        else if constexpr (REP == 2) { below = mn2(med3(lo), min3(mi)); above = mx2(med3(hi), max3(mi)); }
        else {
            const V a1 = med3(lo), a2 = max3(lo), b0 = min3(mi), b2 = max3(mi), c0 = min3(hi), c1 = med3(hi);
            if constexpr (REP == 3) { below = mn2(mx2(a1, b0), mn2(a2, c0)); above = mx2(mn2(c1, b2), mx2(c0, a2)); }
            else { const V b1 = med3(mi); below = mx2(mx2(a1, b0), mn2(mn2(a2, c0), b1)); above = mn2(mn2(c1, b2), mx2(mx2(c0, a2), b1)); }
        }
        e = mn2(mx2(e, below), above);
    }
    return sel(lev, e, c);
}

// lane i takes v of lane i - 1 / i + 1 (lane 0 / 63: 0)
__device__ __forceinline__ uint32_t edge_from_left(uint32_t v) { return __builtin_amdgcn_update_dpp(0u, v, 0x138, 0xF, 0xF, false); }    // wave_shr:1
__device__ __forceinline__ uint32_t edge_from_right(uint32_t v) { return __builtin_amdgcn_update_dpp(0u, v, 0x130, 0xF, 0xF, false); }   // wave_shl:1

// a row of the window: d[1..4] the lane's 16 bytes, d[0] / d[5] the dword before / behind them
struct EdgeRow { uint32_t d[6]; };

// a row of 8-bit containers in halves: pixel q (from the lane's first) is byte q + 4 of the row's 24
struct EdgeSpan8 {
    uint32_t e[6], o[6];
    __device__ __forceinline__ explicit EdgeSpan8(const EdgeRow& r)
    {
#pragma unroll
        for (int k = 0; k < 6; ++k) { e[k] = edge_opaque(r.d[k] & 0x00FF00FFu); o[k] = edge_opaque((r.d[k] >> 8) & 0x00FF00FFu); }
    }
    // pixels (q, q + 2), -4 <= q <= 17
    __device__ __forceinline__ edge_s2 at(int q) const
    {
        const int k = (q + 4) >> 2, r = (q + 4) & 3;
        return __builtin_bit_cast(edge_s2, r == 0 ? e[k] : r == 1 ? o[k] : r == 2 ? __builtin_amdgcn_alignbit(e[k + 1], e[k], 16) : __builtin_amdgcn_alignbit(o[k + 1], o[k], 16));
    }
};

// The lane's 16 bytes of output row y from the window w[0..5) = rows y - 2 .. y + 2, every pixel taken as an interior one
template <typename T, int REP>
__device__ __forceinline__ uint4 edge_cell(const EdgeRow (&w)[5], int thresh, int strength)
{
    uint32_t O[4];
    if constexpr (sizeof(T) == 1) {
        const EdgeSpan8 R0(w[0]), R1(w[1]), R2(w[2]), R3(w[3]), R4(w[4]);
        const edge_s2 thr = EdgeLanes<edge_s2>::splat(thresh);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t res[2];
#pragma unroll
            for (int par = 0; par < 2; ++par) {                                         // the even bytes of dword k, then the odd ones
                const int q = 4 * k + par;
                const edge_s2 h[5] = {R2.at(q - 2), R2.at(q - 1), R2.at(q), R2.at(q + 1), R2.at(q + 2)};
                const edge_s2 v[5] = {R0.at(q), R1.at(q), h[2], R3.at(q), R4.at(q)};
                const edge_s2 u[3] = {R1.at(q - 1), v[1], R1.at(q + 1)}, d[3] = {R3.at(q - 1), v[3], R3.at(q + 1)};
                res[par] = __builtin_bit_cast(uint32_t, edge_pixel<edge_s2, REP>(h, v, u, d, thr, strength));
            }
            O[k] = res[0] | res[1] << 8;                                                // every result lies in 0..255
        }
    } else {
        auto px = [](const EdgeRow& r, int i) { return (int)((r.d[i >> 1] >> (16 * (i & 1))) & 0xFFFFu); };      // container i - 2 from the lane's first
#pragma unroll
        for (int k = 0; k < 4; ++k) O[k] = 0;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const int h[5] = {px(w[2], g), px(w[2], g + 1), px(w[2], g + 2), px(w[2], g + 3), px(w[2], g + 4)};
            const int v[5] = {px(w[0], g + 2), px(w[1], g + 2), h[2], px(w[3], g + 2), px(w[4], g + 2)};
            const int u[3] = {px(w[1], g + 1), v[1], px(w[1], g + 3)}, d[3] = {px(w[3], g + 1), v[3], px(w[3], g + 3)};
            O[g >> 1] |= (uint32_t)edge_pixel<int, REP>(h, v, u, d, thresh, strength) << (16 * (g & 1));       // every result lies in 0..65535
        }
    }
    return uint4{O[0], O[1], O[2], O[3]};
}

} // namespace

} // namespace amt
