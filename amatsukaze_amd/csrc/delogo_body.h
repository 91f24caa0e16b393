// delogo_body.h -- what every Delogo kernel body is made of: AMTEraseLogo::Delogo's arithmetic for one sample, and N adjacent
// containers moved as one access.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "exact_math.h"
#include "pack16.h"

namespace amt {

// AMTEraseLogo::Delogo's arithmetic for one sample (LogoScan.hpp:1253-1259)
__device__ __forceinline__ float delogo_px(float s, float a, float b, float maxv, float fade)
{
    const float bg = unblend_bg(a, b, maxv, s);
    const float t = fade_mix(fade, bg, s) + 0.5f;
    const float lo = (t < 0.0f) ? 0.0f : t;            // std::max(t, 0.0f)
    return (maxv < lo) ? maxv : lo;                    // std::min(lo, maxv)
}

// N adjacent containers as one access: get = their samples (container >> shift), pack = the containers of N results (result << shift).
// 8-bit containers are never shifted
template <typename C, int N> struct Run;
template <> struct Run<uint8_t, 4> {
    typedef uint32_t type;
    static __device__ __forceinline__ void get(type v, int, float (&s)[4])
    {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = (float)((v >> (8 * k)) & 0xFFu);
    }
    static __device__ __forceinline__ type pack(const float (&r)[4], int)
    {
        return (uint32_t)(uint8_t)r[0] | ((uint32_t)(uint8_t)r[1] << 8) | ((uint32_t)(uint8_t)r[2] << 16) | ((uint32_t)(uint8_t)r[3] << 24);
    }
};
template <> struct Run<uint8_t, 2> {
    typedef uint16_t type;
    static __device__ __forceinline__ void get(type v, int, float (&s)[2]) { s[0] = (float)(uint8_t)v; s[1] = (float)(uint8_t)(v >> 8); }
    static __device__ __forceinline__ type pack(const float (&r)[2], int) { return (uint16_t)((uint16_t)(uint8_t)r[0] | ((uint16_t)(uint8_t)r[1] << 8)); }
};
template <> struct Run<uint8_t, 1> {
    typedef uint8_t type;
    static __device__ __forceinline__ void get(type v, int, float (&s)[1]) { s[0] = (float)v; }
    static __device__ __forceinline__ type pack(const float (&r)[1], int) { return (uint8_t)r[0]; }
};
template <> struct Run<uint16_t, 4> {
    typedef uint2 type;
    static __device__ __forceinline__ void get(type v, int shift, float (&s)[4])
    {
        const uint32_t lo = pk_shr16(v.x, shift), hi = pk_shr16(v.y, shift);
        s[0] = (float)(lo & 0xFFFFu); s[1] = (float)(lo >> 16); s[2] = (float)(hi & 0xFFFFu); s[3] = (float)(hi >> 16);
    }
    static __device__ __forceinline__ type pack(const float (&r)[4], int shift)
    {
        return make_uint2(pk_shl16((uint32_t)(uint16_t)r[0] | ((uint32_t)(uint16_t)r[1] << 16), shift),
                          pk_shl16((uint32_t)(uint16_t)r[2] | ((uint32_t)(uint16_t)r[3] << 16), shift));
    }
};
template <> struct Run<uint16_t, 2> {
    typedef uint32_t type;
    static __device__ __forceinline__ void get(type v, int shift, float (&s)[2])
    {
        const uint32_t w = pk_shr16(v, shift);
        s[0] = (float)(w & 0xFFFFu); s[1] = (float)(w >> 16);
    }
    static __device__ __forceinline__ type pack(const float (&r)[2], int shift)
    {
        return pk_shl16((uint32_t)(uint16_t)r[0] | ((uint32_t)(uint16_t)r[1] << 16), shift);
    }
};
template <> struct Run<uint16_t, 1> {
    typedef uint16_t type;
    static __device__ __forceinline__ void get(type v, int shift, float (&s)[1]) { s[0] = (float)(uint16_t)(v >> shift); }
    static __device__ __forceinline__ type pack(const float (&r)[1], int shift) { return (uint16_t)((uint16_t)r[0] << shift); }
};

} // namespace amt
