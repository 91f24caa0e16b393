// pack16.h -- packed operations on the two 16-bit halves of a dword, shared by the kernels that read or write MSB-aligned 16-bit containers
// (P010 / P012: sample = container >> (16 - bits)).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace amt {

// both 16-bit halves of w shifted right by s (one v_pk_lshrrev_b16)
__device__ __forceinline__ uint32_t pk_shr16(uint32_t w, int s)
{
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    us2 v = __builtin_bit_cast(us2, w);
    v >>= (unsigned short)s;
    return __builtin_bit_cast(uint32_t, v);
}

// ... shifted left by s (one v_pk_lshlrev_b16)
__device__ __forceinline__ uint32_t pk_shl16(uint32_t w, int s)
{
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    us2 v = __builtin_bit_cast(us2, w);
    v <<= (unsigned short)s;
    return __builtin_bit_cast(uint32_t, v);
}

} // namespace amt
