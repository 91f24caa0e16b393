// render_body.h -- the packed arithmetic and the row fill of the cadence renderer, one text for the planar LSB
// kernels (render_kernels.hip) and the decoder-surface kernels (render_surface_kernels.hip).  Device code only.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "pack16.h"

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

// every 16-bit container of 16 bytes shifted right by s (pack16.h)
__device__ __forceinline__ uint4 render_pk_shr16(uint4 v, int s) { return uint4{pk_shr16(v.x, s), pk_shr16(v.y, s), pk_shr16(v.z, s), pk_shr16(v.w, s)}; }

// one missing row: nb bytes at d from the rows up / dn (and ta / tb).  The vector form issues the 2 (4) loads of a lane's 16 bytes before
// their first use; the row's last nb % 16 bytes go container by container.  MSB (16-bit containers): the rule runs on the samples
// container >> s (t in sample units), one packed shift per loaded dword, and the result is stored as sample << s, low bits zero
template <int ES, bool VEC, bool TEMPORAL, bool MSB = false>
__device__ __forceinline__ void render_fill_row(uint8_t* d, const uint8_t* up, const uint8_t* dn, const uint8_t* ta, const uint8_t* tb, int nb, int t, int lane,
                                                int s = 0)
{
    static_assert(!MSB || ES == 2, "MSB-aligned samples sit in 16-bit containers");
    typedef typename std::conditional<ES == 1, uint8_t, uint16_t>::type T;
    auto one = [&](int k) {                                                             // the container at byte k
        if constexpr (MSB) {
            // the vector form's arithmetic on one container in the low half of a dword: the same shifts, mean and select
            const uint32_t u = *reinterpret_cast<const T*>(up + k), w = *reinterpret_cast<const T*>(dn + k);
            uint32_t p = u, q = u;
            if constexpr (TEMPORAL) { p = *reinterpret_cast<const T*>(ta + k); q = *reinterpret_cast<const T*>(tb + k); }
            const uint32_t v = render_mix<ES, TEMPORAL>(pk_shr16(u, s), pk_shr16(w, s), pk_shr16(p, s), pk_shr16(q, s), (uint32_t)t);
            *reinterpret_cast<T*>(d + k) = (T)pk_shl16(v, s);
            return;
        }
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
            uint4 u = *reinterpret_cast<const uint4*>(up + x), w = *reinterpret_cast<const uint4*>(dn + x);
            uint4 p = u, q = u;
            if constexpr (TEMPORAL) { p = *reinterpret_cast<const uint4*>(ta + x); q = *reinterpret_cast<const uint4*>(tb + x); }
            if constexpr (MSB) {
                u = render_pk_shr16(u, s); w = render_pk_shr16(w, s);
                if constexpr (TEMPORAL) { p = render_pk_shr16(p, s); q = render_pk_shr16(q, s); }
            }
            uint4 o;
            o.x = render_mix<ES, TEMPORAL>(u.x, w.x, p.x, q.x, (uint32_t)t); o.y = render_mix<ES, TEMPORAL>(u.y, w.y, p.y, q.y, (uint32_t)t);
            o.z = render_mix<ES, TEMPORAL>(u.z, w.z, p.z, q.z, (uint32_t)t); o.w = render_mix<ES, TEMPORAL>(u.w, w.w, p.w, q.w, (uint32_t)t);
            if constexpr (MSB) { o.x = pk_shl16(o.x, s); o.y = pk_shl16(o.y, s); o.z = pk_shl16(o.z, s); o.w = pk_shl16(o.w, s); }
            *reinterpret_cast<uint4*>(d + x) = o;
        }
        for (int k = (nb & ~15) + lane * ES; k < nb; k += 64 * ES) one(k);             // the row's last nb % 16 bytes
    } else {
        for (int k = lane * ES; k < nb; k += 64 * ES) one(k);
    }
}

} // namespace amt
