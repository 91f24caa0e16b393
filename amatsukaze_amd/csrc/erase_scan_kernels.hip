// erase_scan_kernels.hip -- logo erase (Delogo) and logo generation (LogoScan accumulate) kernels.
//
// Both are elementwise / reduction passes over the logo rectangle only (w*h luma + 2*wUV*hUV chroma
// samples per frame): HBM-bound, a few ops per byte.  One workgroup row = one rectangle row so that a
// wave reads/writes one contiguous run of the frame; frames and rows give >> 256 workgroups.
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstdint>

#include "delogo_body.h"
#include "exact_math.h"
#include "kernels.hpp"

namespace amt {

// ------------------------------------------------------------------------------------------------
// AMTEraseLogo::Delogo (LogoScan.hpp:1248-1261) applied as GetFrameT mode 0 does (:1374-1397):
// frame mode when fadeT == fadeB, otherwise per field with chroma row parity (imgy/2)%2.  In field mode
// the reference processes hUV/2 chroma rows per field, so an odd last chroma row is left untouched.
// ------------------------------------------------------------------------------------------------

// One workgroup = kDelogoRows consecutive rectangle rows (luma rows first, then U, then V) of one frame; a
// thread owns PAIRS of horizontally adjacent samples (the rectangle origin and width are even, LogoScan.hpp:69,
// so a luma pair is one aligned 2*sizeof(pix_t) access; chroma pairs are used when the chroma origin, width and
// pitch are even too, otherwise that plane goes sample by sample), for kDelogoFrames consecutive frames: the pass is a
// read-modify-write of 48 KiB per frame against 384 KiB of logo coefficients, which are therefore loaded once per group.
#ifndef AMT_DELOGO_ROWS
#define AMT_DELOGO_ROWS 16
#endif
#ifndef AMT_DELOGO_FRAMES
#define AMT_DELOGO_FRAMES 8
#endif
constexpr int kDelogoRows = AMT_DELOGO_ROWS;
constexpr int kDelogoThreads = 256;
constexpr int kDelogoFrames = AMT_DELOGO_FRAMES;       // frames a workgroup walks through with the row's logo coefficients in registers

// four adjacent samples in one access (rows whose width is a multiple of 4: one wave moves 256 / 512 contiguous bytes per row)
template <typename pix_t> struct PixQuad;
template <> struct PixQuad<uint8_t> {
    typedef uint32_t __attribute__((aligned(2))) type;
    static __device__ __forceinline__ float get(uint32_t v, int k) { return (float)((v >> (8 * k)) & 0xFFu); }
    static __device__ __forceinline__ uint32_t pack(float r0, float r1, float r2, float r3)
    {
        return (uint32_t)(uint8_t)r0 | ((uint32_t)(uint8_t)r1 << 8) | ((uint32_t)(uint8_t)r2 << 16) | ((uint32_t)(uint8_t)r3 << 24);
    }
};
template <> struct PixQuad<uint16_t> {
    typedef uint64_t __attribute__((aligned(4))) type;
    static __device__ __forceinline__ float get(uint64_t v, int k) { return (float)((v >> (16 * k)) & 0xFFFFu); }
    static __device__ __forceinline__ uint64_t pack(float r0, float r1, float r2, float r3)
    {
        return (uint64_t)(uint16_t)r0 | ((uint64_t)(uint16_t)r1 << 16) | ((uint64_t)(uint16_t)r2 << 32) | ((uint64_t)(uint16_t)r3 << 48);
    }
};
template <typename pix_t> struct PixPair;
template <> struct PixPair<uint8_t> { typedef uint16_t type; };
template <> struct PixPair<uint16_t> { typedef uint32_t type; };

template <typename pix_t>
__global__ __launch_bounds__(kDelogoThreads)
void delogo_kernel(const pix_t* sY, const pix_t* sU, const pix_t* sV, pix_t* Y, pix_t* U, pix_t* V, long long strideY,
                   long long strideUV, int pitchY, int pitchUV, const float* __restrict__ planes, EraseGeom g,
                   float maxv, const float2* __restrict__ fades, int pairY, int pairUV, int nframes, int quadY, int quadUV,
                   int zero_identity)
{
    typedef typename PixPair<pix_t>::type pair_t;
    typedef typename PixQuad<pix_t>::type quad_t;
    constexpr int SH = 8 * sizeof(pix_t);
    const int f0 = blockIdx.y * kDelogoFrames;
    const int f1 = min(nframes, f0 + kDelogoFrames);
    const size_t ysz = (size_t)g.w * g.h, csz = (size_t)g.wUV * g.hUV;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (zero_identity) {
        // a group whose frames all carry fade {0, 0} has nothing to rewrite (half of a clip whose logo comes and goes): leave before the
        // coefficient rows are fetched
        bool any = false;
        for (int f = f0; f < f1; ++f) { const float2 fd = fades[f]; any = any || fd.x != 0.0f || fd.y != 0.0f; }
        if (!any) return;
    }
    const int rend = min(g.h + 2 * g.hUV, (int)(blockIdx.x + 1) * kDelogoRows);
    for (int r = blockIdx.x * kDelogoRows + wv; r < rend; r += kDelogoThreads / 64) {
        // the row's geometry and logo coefficients are the same for every frame of the group: the logo planes are
        // 8 B per sample against 2 B of frame traffic, so they are read once and kept in registers
        pix_t* row0;             // the row in the destination batch
        const pix_t* srow0;      // ... in the source batch (the same pointer for the in-place call)
        const float *A, *B;
        int roww, paired, quad, y, pl;
        long long stride;
        if (r < g.h) {
            y = r; pl = 0;
            roww = g.w; paired = pairY; quad = quadY; stride = strideY;
            row0 = Y + (long long)(g.imgy + y) * pitchY + g.imgx;
            srow0 = sY + (long long)(g.imgy + y) * pitchY + g.imgx;
            A = planes + (size_t)y * g.w; B = planes + ysz + (size_t)y * g.w;
        } else {
            pl = (r - g.h) >= g.hUV ? 2 : 1;
            y = r - g.h - (pl - 1) * g.hUV;
            roww = g.wUV; paired = pairUV; quad = quadUV; stride = strideUV;
            row0 = (pl == 2 ? V : U) + (long long)(g.cy + y) * pitchUV + g.cx;
            srow0 = (pl == 2 ? sV : sU) + (long long)(g.cy + y) * pitchUV + g.cx;
            const float* base = planes + 2 * ysz + (size_t)(pl - 1) * 2 * csz;
            A = base + (size_t)y * g.wUV; B = base + csz + (size_t)y * g.wUV;
        }
        auto fade_of = [&](float2 fd, bool& skip) {
            const bool frameMode = fd.x == fd.y;
            skip = pl != 0 && !frameMode && y >= 2 * (g.hUV / 2);   // field mode leaves an odd last chroma row alone
            // fade 0 writes back what it read (0*bg + 1*s + 0.5 truncates to s) whenever bg is finite, which the host has checked
            // for this logo (zero_identity): frames without a logo cost no traffic
            skip = skip || (zero_identity && fd.x == 0.0f && fd.y == 0.0f);
            if (frameMode) return fd.x;
            return pl == 0 ? ((y & 1) ? fd.y : fd.x) : (((y & 1) == g.uvparity) ? fd.x : fd.y);
        };
        if (quad) {
            for (int x = 4 * lane; x < roww; x += 256) {
                const float4 a = *reinterpret_cast<const float4*>(A + x);
                const float4 b = *reinterpret_cast<const float4*>(B + x);
                float fd[kDelogoFrames];
                bool live[kDelogoFrames];
#pragma unroll
                for (int k = 0; k < kDelogoFrames; ++k) {
                    bool skip = true;
                    fd[k] = f0 + k < f1 ? fade_of(fades[f0 + k], skip) : 0.0f;
                    live[k] = !skip;
                }
                typename PixQuad<pix_t>::type v[kDelogoFrames];          // all live frames' loads in flight before the first use
#pragma unroll
                for (int k = 0; k < kDelogoFrames; ++k)
                    if (live[k]) v[k] = *reinterpret_cast<const quad_t*>(srow0 + (long long)(f0 + k) * stride + x);
#pragma unroll
                for (int k = 0; k < kDelogoFrames; ++k) {
                    if (!live[k]) continue;
                    typedef PixQuad<pix_t> Q;
                    const float r0 = delogo_px(Q::get(v[k], 0), a.x, b.x, maxv, fd[k]);
                    const float r1 = delogo_px(Q::get(v[k], 1), a.y, b.y, maxv, fd[k]);
                    const float r2 = delogo_px(Q::get(v[k], 2), a.z, b.z, maxv, fd[k]);
                    const float r3 = delogo_px(Q::get(v[k], 3), a.w, b.w, maxv, fd[k]);
                    *reinterpret_cast<quad_t*>(row0 + (long long)(f0 + k) * stride + x) = Q::pack(r0, r1, r2, r3);
                }
            }
        } else if (paired) {
            for (int x = 2 * lane; x < roww; x += 128) {
                const float2 a = *reinterpret_cast<const float2*>(A + x);
                const float2 b = *reinterpret_cast<const float2*>(B + x);
                pair_t v[kDelogoFrames];                                 // all frames' loads in flight before the first use
#pragma unroll
                for (int k = 0; k < kDelogoFrames; ++k)
                    v[k] = *reinterpret_cast<const pair_t*>(srow0 + (long long)min(f0 + k, f1 - 1) * stride + x);
#pragma unroll
                for (int k = 0; k < kDelogoFrames; ++k) {
                    const int f = f0 + k;
                    if (f >= f1) break;
                    bool skip;
                    const float fade = fade_of(fades[f], skip);
                    if (skip) continue;
                    const float r0 = delogo_px((float)(pix_t)v[k], a.x, b.x, maxv, fade);
                    const float r1 = delogo_px((float)(pix_t)(v[k] >> SH), a.y, b.y, maxv, fade);
                    *reinterpret_cast<pair_t*>(row0 + (long long)f * stride + x) = (pair_t)((pair_t)(pix_t)r0 | ((pair_t)(pix_t)r1 << SH));
                }
            }
        } else {
            for (int x = lane; x < roww; x += 64) {
                const float a = A[x], b = B[x];
                for (int f = f0; f < f1; ++f) {
                    bool skip;
                    const float fade = fade_of(fades[f], skip);
                    if (skip) continue;
                    row0[(long long)f * stride + x] = (pix_t)delogo_px((float)srow0[(long long)f * stride + x], a, b, maxv, fade);
                }
            }
        }
    }
}

// what the kernels of this file take: planar LSB planes of the depth's sample size, whole samples between frames
static bool planar_lsb(const FrameBatch& b, int es) { return b.es == es && !b.interleaved && !b.shift && b.strideY % es == 0 && b.strideUV % es == 0; }

hipError_t launch_delogo(hipStream_t st, int bits, const FrameBatch& src, const PlanesOut& dst, const float* dplanes, EraseGeom g, int nframes,
                         const float2* dfades, int zero_identity)
{
    if (nframes <= 0) return hipSuccess;
    const int es = bits <= 8 ? 1 : 2;
    if (!planar_lsb(src, es)) return hipErrorInvalidValue;
    const int rows = g.h + 2 * g.hUV;
    dim3 grid((unsigned)((rows + kDelogoRows - 1) / kDelogoRows), (unsigned)((nframes + kDelogoFrames - 1) / kDelogoFrames)), block(kDelogoThreads);
    const float maxv = (float)((1 << bits) - 1);
    // a pair access needs 2*es alignment of every row start and an even width (plane bases come from hipMalloc /
    // AviSynth's 64-byte aligned planes; a caller handing odd byte offsets falls back to single samples).  dst is laid out like src
    const long long pitchY = (long long)src.pitchY * es, pitchUV = (long long)src.pitchUV * es;
    const int pairY = delogo_pair_lanes(es, RowsAt{lane_addr(src.Y), 0, src.strideY, pitchY}, RowsAt{lane_addr(dst.Y), 0, src.strideY, pitchY},
                                        (long long)g.imgx * es, (long long)g.w * es);
    const int pairUV = delogo_pair_lanes(es, RowsAt{lane_addr(src.U), lane_addr(src.V), src.strideUV, pitchUV},
                                         RowsAt{lane_addr(dst.U), lane_addr(dst.V), src.strideUV, pitchUV}, (long long)g.cx * es, (long long)g.wUV * es);
    // four samples per lane where a row is a multiple of 4 wide (coefficient rows are then 16-byte aligned float4s)
    const int quadY = pairY && g.w % 4 == 0;
    const int quadUV = pairUV && g.wUV % 4 == 0;
    with_sample_type(bits, [&](auto px) {
        typedef decltype(px) pix_t;
        hipLaunchKernelGGL(delogo_kernel<pix_t>, grid, block, 0, st, (const pix_t*)src.Y, (const pix_t*)src.U, (const pix_t*)src.V, (pix_t*)dst.Y,
                           (pix_t*)dst.U, (pix_t*)dst.V, src.strideY / es, src.strideUV / es, src.pitchY, src.pitchUV, dplanes, g, maxv, dfades, pairY,
                           pairUV, nframes, quadY, quadUV, zero_identity);
    });
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// AMTEraseLogo::CalcFade / CalcFade2 (LogoScan.hpp:1263-1341) for a whole batch: one thread per frame.  The decision reads
// nine analysis records around frame n (the argmin over the 11 fades of p for each; t and b of the centre one) -- 99 + 22 floats
// of a table that is L2 resident -- so this is a latency-sized kernel whose point is that the fades never leave the device:
// analysis -> fades -> Delogo is one stream-ordered chain without a host synchronise in the middle.
// Index arithmetic as decisions.cpp fade_from_analysis: k = clamp(n + i) + i, analyze frame q = clamp(k >> 3), source frame
// clamp(8 q + (k & 7)) -- the AviSynth cache's clamping of the analyze clip's frame number, negative k included.
// ------------------------------------------------------------------------------------------------
// i / 10.0f for i = 0..10 and the two threshold tests of (sum of four argmins) / 40 against 0.3 and 0.7 for every possible sum 0..40,
// all evaluated on the host exactly as the reference writes them (float division, comparison against double literals): the
// kernel itself does no floating-point arithmetic, so nothing depends on the device's division
struct FadeTable { float v[11]; unsigned long long below03, above07; };

__device__ __forceinline__ int argmin11_dev(const float* __restrict__ v)
{
    int best = 0;
    float bv = v[0];
#pragma unroll
    for (int i = 1; i < 11; ++i) {
        const float x = v[i];
        if (x < bv) { bv = x; best = i; }       // strict <: the first minimum wins, NaN never does (as the host loop)
    }
    return best;
}

__global__ __launch_bounds__(128)
void calc_fades_kernel(const float* __restrict__ analysis, int analysis_first, int analysis_count, int num_frames, int first, int nframes,
                       const uint8_t* __restrict__ frame_state /* null = no logoframe file */, int half, FadeTable tab,
                       float2* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nframes) return;
    const int n = first + i;
    const int last = num_frames - 1;
    auto clampf = [&](int v) { return max(0, min(last, v)); };
    if (frame_state) {
        // CalcFade (:1317-1341): a window of maxfade frames in one state -> fade 1 if that state is "logo on", else 0
        const int st0 = frame_state[clampf(n - half)];
        bool uniform = true;
        for (int d = -half + 1; d <= half; ++d) uniform = uniform && frame_state[clampf(n + d)] == st0;
        if (uniform) {
            const float f = frame_state[clampf(n)] == 2 ? 1.0f : 0.0f;
            out[i] = make_float2(f, f);
            return;
        }
    }
    const int nAnalyze = (num_frames + 7) / 8;
    int best[9];
    const float* centre = analysis;
#pragma unroll
    for (int d = -4; d <= 4; ++d) {
        const int k = clampf(n + d) + d;
        const int q = max(0, min(nAnalyze - 1, k >> 3));
        const int src = clampf(q * 8 + (k & 7));
        // the host has checked that every record read lies inside [analysis_first, analysis_first + analysis_count)
        const int rel = max(0, min(analysis_count - 1, src - analysis_first));
        const float* rec = analysis + (size_t)rel * 33;
        best[d + 4] = argmin11_dev(rec);
        if (d == 0) centre = rec;
    }
    const int before = best[3] + best[2] + best[1] + best[0], after = best[5] + best[6] + best[7] + best[8];     // 0..40 each
    auto bit = [](unsigned long long m, int s) { return ((m >> s) & 1ull) != 0; };
    const bool abrupt = (bit(tab.below03, before) && bit(tab.above07, after)) || (bit(tab.above07, before) && bit(tab.below03, after));
    if (abrupt) out[i] = make_float2(tab.v[argmin11_dev(centre + 11)], tab.v[argmin11_dev(centre + 22)]);
    else out[i] = make_float2(tab.v[best[4]], tab.v[best[4]]);
}

hipError_t launch_calc_fades(hipStream_t st, const float* danalysis, int analysis_first, int analysis_count, int num_frames, int first,
                             int nframes, const uint8_t* dstate, int half, float2* dout)
{
    if (nframes <= 0) return hipSuccess;
    FadeTable tab;
    for (int i = 0; i < 11; ++i) tab.v[i] = (float)i / 10.0f;
    tab.below03 = tab.above07 = 0;
    for (int s = 0; s <= 40; ++s) {
        float q = 0;
        q += s;                 // (the sum of four small integers is exact in fp32 whatever the order)
        q /= 40;
        if (q < 0.3) tab.below03 |= 1ull << s;
        if (q > 0.7) tab.above07 |= 1ull << s;
    }
    hipLaunchKernelGGL(calc_fades_kernel, dim3((unsigned)((nframes + 127) / 128)), dim3(128), 0, st, danalysis, analysis_first,
                       analysis_count, num_frames, first, nframes, dstate, half, tab, dout);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// LogoScan::AddFrame, first half (LogoScan.hpp:604-653): the rectangle's border samples of each plane,
// reject when max-min > thy, else background = med_average (:414-428) = (int)((sum of the middle half of
// the sorted samples + nn/2) / nn).  Sorting is replaced by a histogram (exact: the sorted sequence is
// the histogram read out in order).  One workgroup per frame.
// The samples are taken at their real container value, whatever the declared depth (AddFrame is a template over pixel_t and
// knows no depth): a first pass reduces their true min and max and decides, and only an accepted plane is histogrammed, as
// value - base.  An accepted plane's samples span at most thy, so they fit the nbins = 1 << bits bins whenever thy < nbins, which
// the host checks.  The reference keeps the samples in `short`: a 16-bit container value above 32767 enters as its
// two's-complement wrap there, and so it does here.
// out[frame] = {valid, bgY, bgU, bgV}; the backgrounds of a rejected frame are 0
// ------------------------------------------------------------------------------------------------
constexpr int kBorderThreads = 256;

__device__ __forceinline__ int border_value(uint8_t v) { return (int)v; }
__device__ __forceinline__ int border_value(uint16_t v) { return (int)(int16_t)v; }      // tmpY is a std::vector<short>

// false: the plane's border spread exceeds thy (the same answer in every thread).  true: bg = its trimmed mean.
template <typename pix_t>
__device__ bool border_plane(const pix_t* __restrict__ p, int pitch, int w, int h, int nbins, int thy, int* hist,
                             long long* red, int* redi, int& bg)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int kWaves = kBorderThreads / 64;
    int* wmin = redi;                            // per-wave partial results: kWaves entries each
    int* wmax = redi + kWaves;
    int* wcnt = redi + 2 * kWaves;
    for (int i = tid; i < nbins; i += kBorderThreads) hist[i] = 0;
    // pass 1: the true min and max of the border samples.  The first trip's samples (all of them, for a rectangle of up to 256 x 258)
    // stay in registers for pass 2.
    const bool hasRow = tid < w, hasCol = 1 + tid < h - 1;
    int ra = 0, rb = 0, ca = 0, cb = 0;
    int mn = 0x7FFFFFFF, mx = -0x7FFFFFFF - 1;
    if (hasRow) {
        ra = border_value(p[tid]); rb = border_value(p[tid + (long long)(h - 1) * pitch]);
        mn = min(ra, rb); mx = max(ra, rb);
    }
    if (hasCol) {
        ca = border_value(p[(long long)(1 + tid) * pitch]); cb = border_value(p[w - 1 + (long long)(1 + tid) * pitch]);
        mn = min(mn, min(ca, cb)); mx = max(mx, max(ca, cb));
    }
    for (int x = tid + kBorderThreads; x < w; x += kBorderThreads) {
        const int a = border_value(p[x]), b = border_value(p[x + (long long)(h - 1) * pitch]);
        mn = min(mn, min(a, b));
        mx = max(mx, max(a, b));
    }
    for (int y = 1 + tid + kBorderThreads; y < h - 1; y += kBorderThreads) {
        const int a = border_value(p[(long long)y * pitch]), b = border_value(p[w - 1 + (long long)y * pitch]);
        mn = min(mn, min(a, b));
        mx = max(mx, max(a, b));
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        mn = min(mn, __shfl_xor(mn, s));
        mx = max(mx, __shfl_xor(mx, s));
    }
    if (lane == 0) { wmin[wave] = mn; wmax[wave] = mx; }
    __syncthreads();                             // (also: the histogram is cleared)
    mn = wmin[0]; mx = wmax[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) { mn = min(mn, wmin[k]); mx = max(mx, wmax[k]); }
    if (mx - mn > thy) return false;             // abs(front - back) > thy (:638-649)
    // pass 2: histogram of value - base.  A plane inside the declared depth keeps bin == value; otherwise the window
    // [base, base + nbins) is moved so that it ends at the max (or starts at a negative min): the accepted samples lie in
    // [max - thy, max] and thy < nbins
    const int base = mn < 0 ? mn : max(0, mx - (nbins - 1));
    if (hasRow) { atomicAdd(&hist[ra - base], 1); atomicAdd(&hist[rb - base], 1); }
    if (hasCol) { atomicAdd(&hist[ca - base], 1); atomicAdd(&hist[cb - base], 1); }
    for (int x = tid + kBorderThreads; x < w; x += kBorderThreads) {
        atomicAdd(&hist[border_value(p[x]) - base], 1);
        atomicAdd(&hist[border_value(p[x + (long long)(h - 1) * pitch]) - base], 1);
    }
    for (int y = 1 + tid + kBorderThreads; y < h - 1; y += kBorderThreads) {
        atomicAdd(&hist[border_value(p[(long long)y * pitch]) - base], 1);
        atomicAdd(&hist[border_value(p[w - 1 + (long long)y * pitch]) - base], 1);
    }
    __syncthreads();
    const int n = 2 * w + 2 * max(0, h - 2);     // a one-row plane (chroma of a 2-row rectangle) pushes its row twice (:616-635)
    const int lo = n / 4, hi = n - n / 4;
    // each thread owns nbins/256 consecutive bins; exclusive prefix of the per-thread counts: a scan inside the wave, the waves'
    // totals through LDS
    const int per = (nbins + kBorderThreads - 1) / kBorderThreads;
    const int b0 = tid * per, b1 = min(nbins, b0 + per);
    int cnt = 0;
    for (int b = b0; b < b1; ++b) cnt += hist[b];
    int incl = cnt;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int v = __shfl_up(incl, s);
        if (lane >= s) incl += v;
    }
    if (lane == 63) wcnt[wave] = incl;
    __syncthreads();
    int before = incl - cnt;
    for (int k = 0; k < wave; ++k) before += wcnt[k];
    long long part = 0;
    int cum = before;
    for (int b = b0; b < b1; ++b) {
        const int c = hist[b];
        if (c) {
            const int s = max(cum, lo), e = min(cum + c, hi);
            if (e > s) part += (long long)(e - s) * (b + base);
        }
        cum += c;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) part += __shfl_xor(part, s);
    if (lane == 0) red[wave] = part;
    __syncthreads();
    long long sum = red[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) sum += red[k];
    const int nn = hi - lo;
    double t = (double)sum;
    t = (t + nn / 2) / nn;
    bg = (int)t;
    // (no barrier here: the next plane writes wmin / wmax, wcnt and red only behind barriers of its own that every thread passes
    // after these reads, and clears the histogram, last read before the barrier above)
    return true;
}

template <typename pix_t>
__global__ __launch_bounds__(kBorderThreads)
void scan_border_kernel(const pix_t* __restrict__ Y, const pix_t* __restrict__ U, const pix_t* __restrict__ V,
                        long long strideY, long long strideUV, int pitchY, int pitchUV, int imgx, int imgy, int cx, int cy,
                        int w, int h, int wUV, int hUV, int nbins, int thy, int4* __restrict__ out)
{
    extern __shared__ int sh[];
    int* hist = sh;                                        // nbins
    int* redi = hist + nbins;                              // 2*256
    long long* red = (long long*)(redi + 2 * kBorderThreads);   // 256 (8-byte aligned: nbins is a multiple of 2)
    const int frame = blockIdx.x;
    int bgY = 0, bgU = 0, bgV = 0;
    // the reference returns at the first plane that fails; the verdict is the same in every thread, so the rest is skipped whole
    const bool ok =
        border_plane(Y + (long long)frame * strideY + (long long)imgy * pitchY + imgx, pitchY, w, h, nbins, thy, hist, red, redi, bgY) &&
        border_plane(U + (long long)frame * strideUV + (long long)cy * pitchUV + cx, pitchUV, wUV, hUV, nbins, thy, hist, red, redi, bgU) &&
        border_plane(V + (long long)frame * strideUV + (long long)cy * pitchUV + cx, pitchUV, wUV, hUV, nbins, thy, hist, red, redi, bgV);
    if (!ok) bgY = bgU = bgV = 0;
    if (threadIdx.x == 0) out[frame] = make_int4(ok ? 1 : 0, bgY, bgU, bgV);
}

hipError_t launch_scan_border(hipStream_t st, int bits, const FrameBatch& b, const ScanRect& r, int thy, int nframes, int4* dout)
{
    if (nframes <= 0) return hipSuccess;
    const int es = bits <= 8 ? 1 : 2;
    if (!planar_lsb(b, es)) return hipErrorInvalidValue;
    const int nbins = 1 << bits;
    const size_t lds = (size_t)nbins * 4 + 2 * kBorderThreads * 4 + kBorderThreads * 8;
    dim3 grid((unsigned)nframes), block(kBorderThreads);
    with_sample_type(bits, [&](auto px) {
        typedef decltype(px) pix_t;
        hipLaunchKernelGGL(scan_border_kernel<pix_t>, grid, block, lds, st, (const pix_t*)b.Y, (const pix_t*)b.U, (const pix_t*)b.V, b.strideY / es,
                           b.strideUV / es, b.pitchY, b.pitchUV, r.imgx, r.imgy, r.cx, r.cy, r.w, r.h, r.wUV, r.hUV, nbins, thy, dout);
    });
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// LogoScan::AddScanFrame (LogoScan.hpp:568-592) over the accepted frames of a batch.  The reference
// keeps five double sums per pixel; F, F*F and F*B of integer samples are exact integers, so int64
// accumulation gives the same values in any order (and lets shards be all-reduced exactly).  sumB and
// sumB2 are per-plane constants of the accepted set and are kept by the host.
// acc: 3 int64 per pixel {sumF, sumF2, sumFB}; pixels = Y rows, then U rows, then V rows.
// ------------------------------------------------------------------------------------------------
// Frames are split over blockIdx.y so that the launch has a few thousand workgroups, no more: every workgroup ends with
// three 64-bit atomics per pixel, and with a fixed 32 frames per workgroup those atomics (not the 1 B/pixel/frame of
// reads) were the whole cost of a 20000-frame accumulate.
constexpr int kAccMinFramesPerBlock = 32;
constexpr int kAccFrameChunks = 16;

template <typename pix_t>
__global__ __launch_bounds__(256)
void scan_accumulate_kernel(const pix_t* __restrict__ Y, const pix_t* __restrict__ U, const pix_t* __restrict__ V,
                            long long strideY, long long strideUV, int pitchY, int pitchUV, int imgx, int imgy, int cx, int cy,
                            int w, int h, int wUV, int hUV, const int4* __restrict__ accepted /* {frame, bgY, bgU, bgV} */,
                            int naccepted, int frames_per_block, unsigned long long* __restrict__ acc)
{
    const int r = blockIdx.x;
    const int g0 = blockIdx.y * frames_per_block;
    const int g1 = min(naccepted, g0 + frames_per_block);
    const pix_t* base;
    long long stride;
    int roww, pl;
    size_t pix0;
    if (r < h) {
        pl = 0; roww = w; stride = strideY;
        base = Y + (long long)(imgy + r) * pitchY + imgx;
        pix0 = (size_t)r * w;
    } else {
        pl = (r - h) >= hUV ? 2 : 1;
        const int y = r - h - (pl - 1) * hUV;
        roww = wUV; stride = strideUV;
        base = (pl == 1 ? U : V) + (long long)(cy + y) * pitchUV + cx;
        pix0 = (size_t)w * h + (size_t)(pl - 1) * wUV * hUV + (size_t)y * wUV;
    }
    for (int x = threadIdx.x; x < roww; x += blockDim.x) {
        long long sF = 0, sF2 = 0, sFB = 0;
#pragma unroll 8
        for (int i = g0; i < g1; ++i) {
            const int4 a = accepted[i];
            const int f = base[(long long)a.x * stride + x];
            const int b = pl == 0 ? a.y : (pl == 1 ? a.z : a.w);
            sF += f;
            sF2 += (unsigned)f * (unsigned)f;          // (a 16-bit container value squared needs all 32 bits)
            sFB += f * b;
        }
        unsigned long long* o = acc + (pix0 + x) * 3;
        atomicAdd(o + 0, (unsigned long long)sF);
        atomicAdd(o + 1, (unsigned long long)sF2);
        atomicAdd(o + 2, (unsigned long long)sFB);
    }
}

hipError_t launch_scan_accumulate(hipStream_t st, int bits, const FrameBatch& b, const ScanRect& r, const int4* daccepted, int naccepted,
                                  unsigned long long* dacc)
{
    if (naccepted <= 0) return hipSuccess;
    const int es = bits <= 8 ? 1 : 2;
    if (!planar_lsb(b, es)) return hipErrorInvalidValue;
    const int per = std::max(kAccMinFramesPerBlock, (naccepted + kAccFrameChunks - 1) / kAccFrameChunks);
    dim3 grid((unsigned)(r.h + 2 * r.hUV), (unsigned)((naccepted + per - 1) / per)), block(256);
    with_sample_type(bits, [&](auto px) {
        typedef decltype(px) pix_t;
        hipLaunchKernelGGL(scan_accumulate_kernel<pix_t>, grid, block, 0, st, (const pix_t*)b.Y, (const pix_t*)b.U, (const pix_t*)b.V, b.strideY / es,
                           b.strideUV / es, b.pitchY, b.pitchUV, r.imgx, r.imgy, r.cx, r.cy, r.w, r.h, r.wUV, r.hUV, daccepted, naccepted, per, dacc);
    });
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// The streamed ScanLogo's store (InitialLogoCreator::onFrame keeps every accepted frame's rectangle, LogoScan.hpp:899-903): the
// rectangles of the `nkeep` frames of a batch listed in `keep` (batch-local indices, ascending) go to consecutive slots of the tight
// store, Y [slot][h][w], U / V [slot][h/2][w/2], all three planes of all listed frames in one launch.  A pure HBM copy addressed like
// ingest_rows_kernel, in BYTES whatever the sample size es (1 or 2): a row's lanes sit on consecutive bytes, one lane moves 16 bytes
// where the plane's base, stride, pitch, origin and row length are all multiples of 16, else 4, else one sample (es) -- decided per
// plane kind (luma / chroma) by the launcher, so an odd chroma origin costs the luma rows nothing.
// ------------------------------------------------------------------------------------------------
struct ScanKeepArgs {
    const uint8_t *srcY, *srcU, *srcV;     // the rectangle's first sample in frame 0 of the batch
    long long strideY, strideUV;           // bytes between frames
    int pitchY, pitchUV;                   // bytes between rows
    uint8_t *dstY, *dstU, *dstV;           // the first free slot of the store
    int rowY, h, rowC, hUV;                // row lengths in bytes (w * es, wUV * es)
    int vbY, vbC;                          // bytes one lane moves in a luma / chroma row (16, 4 or es)
    int vrowY, vrowC;                      // rowY / vbY, rowC / vbC
    int vecsY, vecsC;                      // vrowY * h, vrowC * hUV
};

__device__ __forceinline__ void keep_vec(uint8_t* d, const uint8_t* s, int vb)
{
    if (vb == 16) *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
    else if (vb == 4) *reinterpret_cast<uint32_t*>(d) = *reinterpret_cast<const uint32_t*>(s);
    else if (vb == 2) *reinterpret_cast<uint16_t*>(d) = *reinterpret_cast<const uint16_t*>(s);
    else *d = *s;
}

__global__ __launch_bounds__(256)
void scan_keep_kernel(ScanKeepArgs a, const int* __restrict__ keep, long long total_vecs)
{
    const int per_frame = a.vecsY + 2 * a.vecsC;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total_vecs; i += (long long)gridDim.x * blockDim.x) {
        const int slot = (int)(i / per_frame);
        int v = (int)(i - (long long)slot * per_frame);
        const long long frame = keep[slot];
        if (v < a.vecsY) {
            const int y = v / a.vrowY, x = (v - y * a.vrowY) * a.vbY;
            keep_vec(a.dstY + ((long long)slot * a.h + y) * a.rowY + x, a.srcY + frame * a.strideY + (long long)y * a.pitchY + x, a.vbY);
        } else {
            v -= a.vecsY;
            const bool second = v >= a.vecsC;
            if (second) v -= a.vecsC;
            const int y = v / a.vrowC, x = (v - y * a.vrowC) * a.vbC;
            keep_vec((second ? a.dstV : a.dstU) + ((long long)slot * a.hUV + y) * a.rowC + x,
                     (second ? a.srcV : a.srcU) + frame * a.strideUV + (long long)y * a.pitchUV + x, a.vbC);
        }
    }
}

hipError_t launch_scan_keep(hipStream_t st, const FrameBatch& b, const ScanRect& r, const int* dkeep, int nkeep, const PlanesOut& store,
                            long long first_slot)
{
    if (nkeep <= 0 || r.w <= 0 || r.h <= 0) return hipSuccess;
    const int es = b.es;
    if ((es != 1 && es != 2) || !planar_lsb(b, es)) return hipErrorInvalidValue;
    ScanKeepArgs a;
    // (the batch's pitches are in samples; everything below is in bytes)
    a.strideY = b.strideY; a.strideUV = b.strideUV;
    const long long pitchY = (long long)b.pitchY * es, pitchUV = (long long)b.pitchUV * es;
    if (pitchY > INT_MAX || pitchUV > INT_MAX) return hipErrorInvalidValue;
    a.pitchY = (int)pitchY; a.pitchUV = (int)pitchUV;
    a.srcY = (const uint8_t*)b.Y + (long long)r.imgy * pitchY + (long long)r.imgx * es;
    a.srcU = (const uint8_t*)b.U + (long long)r.cy * pitchUV + (long long)r.cx * es;
    a.srcV = (const uint8_t*)b.V + (long long)r.cy * pitchUV + (long long)r.cx * es;
    a.rowY = r.w * es; a.h = r.h; a.rowC = r.wUV * es; a.hUV = r.hUV;
    a.dstY = (uint8_t*)store.Y + first_slot * a.rowY * r.h;
    a.dstU = (uint8_t*)store.U + first_slot * a.rowC * r.hUV;
    a.dstV = (uint8_t*)store.V + first_slot * a.rowC * r.hUV;
    // a slot's rows start at multiples of the row length from the store's base, so the row length covers the destination's alignment too
    a.vbY = scan_keep_lane_bytes(es, RowsAt{lane_addr(a.srcY), 0, a.strideY, a.pitchY}, lane_addr(store.Y), 0, a.rowY);
    a.vbC = scan_keep_lane_bytes(es, RowsAt{lane_addr(a.srcU), lane_addr(a.srcV), a.strideUV, a.pitchUV}, lane_addr(store.U), lane_addr(store.V), a.rowC);
    a.vrowY = a.rowY / a.vbY; a.vrowC = a.rowC / a.vbC;
    a.vecsY = a.vrowY * r.h; a.vecsC = a.vrowC * r.hUV;
    const long long total = (long long)(a.vecsY + 2 * a.vecsC) * nkeep;
    if (total <= 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(scan_keep_kernel, dim3(grid), dim3(256), 0, st, a, dkeep, total);
    return hipGetLastError();
}

} // namespace amt
