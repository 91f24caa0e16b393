// surface_kernels.hip -- a rectangle of decoder surfaces (NV12, P010 / P012, planar MSB) as the planar LSB planes everything downstream takes.
//
// A hardware decoder hands out an 8-bit Y plane plus one interleaved U0 V0 U1 V1 ... plane (NV12), or the same layout in 16-bit containers
// with the sample in the HIGH bits (P010 / P012).  ScanLogo only ever reads the logo rectangle, so instead of planarising whole frames
// (weave_fields_kernel: 2 * 1.5 * W * H bytes per frame) this pulls the rectangle alone: w x h luma and w/2 x h/2 of each chroma plane per
// frame, sample = container >> shift (shift = 16 - bits for MSB-aligned input, else 0: whatever sits in the low bits is dropped).
//
// Shaped like scan_keep_kernel (erase_scan_kernels.hip): a pure HBM copy addressed in BYTES, all planes of all frames of a batch in one
// launch, a row's lanes on consecutive source bytes.  One lane LOADS 16 bytes where the source's base, stride, pitch, the rectangle's
// origin and row length (and the destination's base, stride and pitch, for what it stores) are multiples of it, else 4 bytes, else one
// sample -- decided per plane kind (luma / chroma) by the launcher.  The lanes of a row tile it exactly (row bytes / lane bytes of them):
// no load is rounded up, so a rectangle that ends on the last sample of an unpadded surface reads nothing behind it.
// Interleaved chroma is split in registers: v_perm_b32 picks the even / odd bytes (8-bit) or half-words (16-bit) of two loaded dwords,
// so one lane's load feeds one U store and one V store of half its width each.  The MSB shift is one v_pk_lshrrev_b16 per loaded dword,
// before the split.  No LDS, no scratch.
//
// Latency-sized: 75 KB in and 50 KB out per frame for a 256 x 128 rectangle of NV12 -- a 64-frame batch is 8 MB and a few microseconds
// of HBM time, the size of a launch.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdint>

#include "kernels.hpp"
#include "pack16.h"

namespace amt {

struct SurfaceExtractArgs {
    const uint8_t *srcY, *srcU, *srcV;     // the rectangle's first sample in picture 0 (interleaved: srcU = its first U V pair, srcV unused)
    long long sstrideY, sstrideUV;         // bytes between pictures
    int spitchY, spitchUV;                 // bytes between source rows
    uint8_t *dstY, *dstU, *dstV;
    long long dstrideY, dstrideUV;         // bytes between frames
    int dpitchY, dpitchUV;                 // bytes between destination rows
    int h, hUV;
    int vbY, vbC;                          // bytes one lane LOADS in a luma / chroma row (16, 4 or es; interleaved chroma: 16, 4 or 2 * es as two loads)
    int vrowY, vrowC;                      // lanes per luma / chroma source row
    int vecsY, vecsC;                      // vrowY * h, vrowC * hUV
    int es, interleaved, shift;            // bytes per sample; chroma as U V pairs; right shift of every 16-bit container
    int pairC;                             // interleaved chroma goes pair by pair (two loads of one sample: vbC = 2 * es is then no load width)
};

// even / odd bytes (es 1) or half-words (es 2) of the 8 bytes {lo, hi}
__device__ __forceinline__ uint32_t split_first(uint32_t lo, uint32_t hi, int es)
{
    return es == 1 ? __builtin_amdgcn_perm(hi, lo, 0x06040200u) : __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}
__device__ __forceinline__ uint32_t split_second(uint32_t lo, uint32_t hi, int es)
{
    return es == 1 ? __builtin_amdgcn_perm(hi, lo, 0x07050301u) : __builtin_amdgcn_perm(hi, lo, 0x07060302u);
}

// vb bytes at s to d, every 16-bit container shifted right by `shift` (0 for 8-bit samples)
__device__ __forceinline__ void extract_vec(uint8_t* d, const uint8_t* s, int vb, int shift)
{
    if (vb == 16) {
        uint4 q = *reinterpret_cast<const uint4*>(s);
        q.x = pk_shr16(q.x, shift); q.y = pk_shr16(q.y, shift); q.z = pk_shr16(q.z, shift); q.w = pk_shr16(q.w, shift);
        *reinterpret_cast<uint4*>(d) = q;
    } else if (vb == 4) {
        *reinterpret_cast<uint32_t*>(d) = pk_shr16(*reinterpret_cast<const uint32_t*>(s), shift);
    } else if (vb == 2) {
        *reinterpret_cast<uint16_t*>(d) = (uint16_t)(*reinterpret_cast<const uint16_t*>(s) >> shift);
    } else {
        *d = *s;
    }
}

// vb bytes of U V pairs at s: the U samples to dU, the V samples to dV (vb / 2 bytes each)
__device__ __forceinline__ void extract_split(uint8_t* dU, uint8_t* dV, const uint8_t* s, int vb, int es, int shift, int pairwise)
{
    if (pairwise) {
        if (es == 2) {
            *reinterpret_cast<uint16_t*>(dU) = (uint16_t)(reinterpret_cast<const uint16_t*>(s)[0] >> shift);
            *reinterpret_cast<uint16_t*>(dV) = (uint16_t)(reinterpret_cast<const uint16_t*>(s)[1] >> shift);
        } else {
            *dU = s[0];
            *dV = s[1];
        }
    } else if (vb == 16) {
        uint4 q = *reinterpret_cast<const uint4*>(s);
        q.x = pk_shr16(q.x, shift); q.y = pk_shr16(q.y, shift); q.z = pk_shr16(q.z, shift); q.w = pk_shr16(q.w, shift);
        *reinterpret_cast<uint2*>(dU) = make_uint2(split_first(q.x, q.y, es), split_first(q.z, q.w, es));
        *reinterpret_cast<uint2*>(dV) = make_uint2(split_second(q.x, q.y, es), split_second(q.z, q.w, es));
    } else {
        // one pair of 16-bit samples, or two pairs of bytes: the split of {w, w} has the lane's samples in its low half
        const uint32_t w = pk_shr16(*reinterpret_cast<const uint32_t*>(s), shift);
        *reinterpret_cast<uint16_t*>(dU) = (uint16_t)(es == 1 ? split_first(w, w, 1) : w);
        *reinterpret_cast<uint16_t*>(dV) = (uint16_t)(es == 1 ? split_second(w, w, 1) : w >> 16);
    }
}

__global__ __launch_bounds__(256)
void surfaces_extract_kernel(SurfaceExtractArgs a, long long total_vecs)
{
    // planar chroma: U rows then V rows, vecsC lanes each; interleaved: vecsC lanes that each feed both planes
    const int per_frame = a.vecsY + (a.interleaved ? a.vecsC : 2 * a.vecsC);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total_vecs; i += (long long)gridDim.x * blockDim.x) {
        const long long frame = i / per_frame;
        int v = (int)(i - frame * per_frame);
        if (v < a.vecsY) {
            const int y = v / a.vrowY, x = (v - y * a.vrowY) * a.vbY;
            extract_vec(a.dstY + frame * a.dstrideY + (long long)y * a.dpitchY + x, a.srcY + frame * a.sstrideY + (long long)y * a.spitchY + x, a.vbY,
                        a.shift);
        } else if (a.interleaved) {
            v -= a.vecsY;
            const int y = v / a.vrowC, x = (v - y * a.vrowC) * a.vbC;
            const long long d = frame * a.dstrideUV + (long long)y * a.dpitchUV + (x >> 1);
            extract_split(a.dstU + d, a.dstV + d, a.srcU + frame * a.sstrideUV + (long long)y * a.spitchUV + x, a.vbC, a.es, a.shift, a.pairC);
        } else {
            v -= a.vecsY;
            const bool second = v >= a.vecsC;
            if (second) v -= a.vecsC;
            const int y = v / a.vrowC, x = (v - y * a.vrowC) * a.vbC;
            extract_vec((second ? a.dstV : a.dstU) + frame * a.dstrideUV + (long long)y * a.dpitchUV + x,
                        (second ? a.srcV : a.srcU) + frame * a.sstrideUV + (long long)y * a.spitchUV + x, a.vbC, a.shift);
        }
    }
}

hipError_t launch_surfaces_extract(hipStream_t st, const FrameBatch& s, const ScanRect& r, int nframes, const PlanesOut& dst, long long dstrideY,
                                   long long dstrideUV, int dpitchY, int dpitchUV)
{
    if (nframes <= 0 || r.w <= 0 || r.h <= 0) return hipSuccess;
    const int es = s.es, il = s.interleaved ? 1 : 0;
    if ((es != 1 && es != 2) || (es == 1 && s.shift) || s.shift < 0 || s.shift > 7) return hipErrorInvalidValue;
    SurfaceExtractArgs a;
    // (the descriptor's strides are in bytes, its pitches in containers; everything below is in bytes)
    const long long spitchY = (long long)s.pitchY * es, spitchUV = (long long)s.pitchUV * es;
    const long long dpY = (long long)dpitchY * es, dpUV = (long long)dpitchUV * es;
    if (spitchY > INT_MAX || spitchUV > INT_MAX || dpY > INT_MAX || dpUV > INT_MAX) return hipErrorInvalidValue;
    a.sstrideY = s.strideY; a.sstrideUV = s.strideUV;
    a.spitchY = (int)spitchY; a.spitchUV = (int)spitchUV;
    a.srcY = (const uint8_t*)s.Y + (long long)r.imgy * spitchY + (long long)r.imgx * es;
    // an interleaved row holds the pair of chroma sample x at container 2 x
    a.srcU = (const uint8_t*)s.U + (long long)r.cy * spitchUV + (long long)r.cx * es * (il ? 2 : 1);
    a.srcV = il ? nullptr : (const uint8_t*)s.V + (long long)r.cy * spitchUV + (long long)r.cx * es;
    a.dstY = (uint8_t*)dst.Y; a.dstU = (uint8_t*)dst.U; a.dstV = (uint8_t*)dst.V;
    a.dstrideY = dstrideY; a.dstrideUV = dstrideUV;
    a.dpitchY = (int)dpY; a.dpitchUV = (int)dpUV;
    a.h = r.h; a.hUV = r.hUV;
    a.es = es; a.interleaved = il; a.shift = s.shift;
    const int rowY = r.w * es, rowC = r.wUV * es * (il ? 2 : 1);          // SOURCE bytes of a rectangle row
    a.vbY = extract_lane_bytes(es, RowsAt{lane_addr(a.srcY), 0, a.sstrideY, a.spitchY}, RowsAt{lane_addr(a.dstY), 0, a.dstrideY, a.dpitchY}, rowY);
    const RowsAt srcC{lane_addr(a.srcU), lane_addr(a.srcV), a.sstrideUV, a.spitchUV}, dstC{lane_addr(a.dstU), lane_addr(a.dstV), a.dstrideUV, a.dpitchUV};
    const SplitLanes split = extract_split_lanes(es, srcC, dstC, rowC);
    a.vbC = il ? split.bytes : extract_lane_bytes(es, srcC, dstC, rowC);
    a.pairC = il ? split.pairwise : 0;
    a.vrowY = rowY / a.vbY; a.vrowC = rowC / a.vbC;
    a.vecsY = a.vrowY * r.h; a.vecsC = a.vrowC * r.hUV;
    const long long total = (long long)(a.vecsY + (il ? 1 : 2) * a.vecsC) * nframes;
    if (total <= 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(surfaces_extract_kernel, dim3(grid), dim3(256), 0, st, a, total);
    return hipGetLastError();
}

} // namespace amt
