// logofind_body.h -- the logo finder's kernel template (logofind_kernels.hip has the description), shared by its plain form and the
// form for MSB-aligned samples (logofind_msb_kernels.hip), which lives in a file of its own so that the plain kernels' code does not
// depend on it.
#pragma once

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace amt {

constexpr int kLfRows = 8;              // rows of a tile (R); a lane loads R + 2
constexpr int kLfLaneCols = 4;          // samples of a row a lane owns
constexpr int kLfSpan = 62 * kLfLaneCols;   // columns a wave owns (lanes 1..62)
constexpr int kLfMinSliceFrames = 512;  // frames a slice walks at least: its flush (16 B of atomics per pixel) stays a few per cent

template <int ES> struct LfRow { unsigned w[ES]; };      // one lane's 4 samples of a row: 1 dword (8-bit) or 2 (16-bit)

template <int ES> __device__ __forceinline__ unsigned lf_sample(const LfRow<ES>& r, int i)
{
    if constexpr (ES == 1) return i == 0 ? (r.w[0] & 0xFFu) : i == 3 ? (r.w[0] >> 24) : ((r.w[0] >> (8 * i)) & 0xFFu);
    else return (i & 1) ? (r.w[i >> 1] >> 16) : (r.w[i >> 1] & 0xFFFFu);
}
// the sample left of this lane's first (the last sample of lane - 1) and right of its last (the first sample of lane + 1)
template <int ES> __device__ __forceinline__ unsigned lf_left(const LfRow<ES>& r)
{
    const unsigned v = (unsigned)__builtin_amdgcn_update_dpp(0, (int)r.w[ES - 1], 0x138, 0xF, 0xF, false);     // wave_shr:1
    return ES == 1 ? v >> 24 : v >> 16;
}
template <int ES> __device__ __forceinline__ unsigned lf_right(const LfRow<ES>& r)
{
    const unsigned v = (unsigned)__builtin_amdgcn_update_dpp(0, (int)r.w[0], 0x130, 0xF, 0xF, false);          // wave_shl:1
    return ES == 1 ? v & 0xFFu : v & 0xFFFFu;
}
// |a - b| + acc for samples below 2^16 (the upper halves are zero)
__device__ __forceinline__ unsigned lf_sad(unsigned a, unsigned b, unsigned acc) { return __builtin_amdgcn_sad_u16(a, b, acc); }

// both 16-bit halves of w shifted right by s
__device__ __forceinline__ unsigned lf_pk_shr16(unsigned w, int s)
{
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    us2 v = __builtin_bit_cast(us2, w);
    v >>= (unsigned short)s;
    return __builtin_bit_cast(unsigned, v);
}

// BUF: every lane column ends inside the row's pitch, rows come in through raw buffer loads (a frame is a buffer of H * pitch bytes:
// rows above and below the frame read as zeros).  Otherwise (an unpadded pitch that is not a multiple of 4 samples) sample by sample.
// MSB (16-bit containers only): every sample is its container >> shift, one packed 16-bit shift per loaded dword; without it `shift` is unused
// and the code is the plain kernel's.
template <int ES, bool BUF, bool MSB>
__global__ __launch_bounds__(64)
void logofind_kernel(const uint8_t* __restrict__ Y, long long frame_stride, int pitch_bytes, int W, int H, int nframes, int slice_frames,
                     int col_waves, unsigned long long* __restrict__ S1, unsigned long long* __restrict__ SM, int shift)
{
    static_assert(!MSB || ES == 2, "MSB-aligned samples live in 16-bit containers");
    constexpr int R = kLfRows, NR = kLfRows + 2;
    const int lane = threadIdx.x;
    const int tile = blockIdx.x / col_waves;
    const int x0 = (blockIdx.x - tile * col_waves) * kLfSpan + (lane - 1) * kLfLaneCols;      // first column of this lane (-4 for lane 0 of span 0)
    const int y0 = tile * R;
    const int n0 = blockIdx.y * slice_frames;
    const int n1 = min(nframes, n0 + slice_frames);
    const unsigned frame_bytes = (unsigned)H * (unsigned)pitch_bytes;
    const unsigned voff = (unsigned)(y0 - 1) * (unsigned)pitch_bytes + (unsigned)(x0 * ES);  // row y0 - 1 (wraps for the first tile: zeros)

    auto load = [&](const uint8_t* frame, LfRow<ES>* rows) {
        if constexpr (BUF) {
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(frame), 0, (int)frame_bytes, 0x00027000);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int off = (int)(voff + (unsigned)(r * pitch_bytes));
                if constexpr (ES == 1) {
                    rows[r].w[0] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0);
                } else {
                    typedef unsigned u2 __attribute__((ext_vector_type(2)));
                    const u2 v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, 0, 0);
                    rows[r].w[0] = v[0];
                    rows[r].w[1] = v[1];
                }
            }
            if constexpr (MSB) {
#pragma unroll
                for (int r = 0; r < NR; ++r)
#pragma unroll
                    for (int k = 0; k < ES; ++k) rows[r].w[k] = lf_pk_shr16(rows[r].w[k], shift);
            }
        } else {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int y = y0 - 1 + r;
#pragma unroll
                for (int k = 0; k < ES; ++k) rows[r].w[k] = 0;
                if (y < 0 || y >= H) continue;
                const uint8_t* row = frame + (long long)y * pitch_bytes;
#pragma unroll
                for (int i = 0; i < kLfLaneCols; ++i) {
                    const int x = x0 + i;
                    if (x < 0 || x >= W) continue;
                    unsigned v = ES == 1 ? row[x] : reinterpret_cast<const uint16_t*>(row)[x];
                    if constexpr (MSB) v >>= shift;
                    if constexpr (ES == 1) rows[r].w[0] |= v << (8 * i);
                    else rows[r].w[i >> 1] |= v << (16 * (i & 1));
                }
            }
        }
    };

    unsigned s1[R][kLfLaneCols], sm[R][kLfLaneCols];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < kLfLaneCols; ++i) s1[r][i] = sm[r][i] = 0;

    // INTERIOR (every row of the tile in 1..H-2: all tiles but the first and last) drops the per-row test, and with it the register
    // copies the compiler places around each conditional row
    auto accumulate = [&](auto interior, const LfRow<ES>* rows) {
        // a sliding window of three unpacked rows: above, this, below
        unsigned up[kLfLaneCols], cur[kLfLaneCols], dn[kLfLaneCols];
#pragma unroll
        for (int i = 0; i < kLfLaneCols; ++i) { up[i] = lf_sample<ES>(rows[0], i); cur[i] = lf_sample<ES>(rows[1], i); }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int y = y0 + r;                      // (rows outside 1..H-2 are uniform over the wave: the branch costs nothing)
#pragma unroll
            for (int i = 0; i < kLfLaneCols; ++i) { dn[i] = lf_sample<ES>(rows[r + 2], i); s1[r][i] += cur[i]; }
            if (decltype(interior)::value || (y >= 1 && y <= H - 2)) {
                const unsigned L = lf_left<ES>(rows[r + 1]), Rt = lf_right<ES>(rows[r + 1]);
#pragma unroll
                for (int i = 0; i < kLfLaneCols; ++i) {
                    const unsigned a = i == 0 ? L : cur[i - 1], b = i == kLfLaneCols - 1 ? Rt : cur[i + 1];
                    sm[r][i] = lf_sad(up[i], dn[i], lf_sad(a, b, sm[r][i]));
                }
            }
#pragma unroll
            for (int i = 0; i < kLfLaneCols; ++i) { up[i] = cur[i]; cur[i] = dn[i]; }
        }
    };

    // two row sets that swap roles: the next frame's loads are in flight while this one is summed
    auto walk = [&](auto interior) {
        LfRow<ES> A[NR], B[NR];
        if (n0 < n1) load(Y + (long long)n0 * frame_stride, A);
        for (int n = n0; n < n1; n += 2) {
            if (n + 1 < n1) load(Y + (long long)(n + 1) * frame_stride, B);
            accumulate(interior, A);
            if (n + 1 >= n1) break;
            if (n + 2 < n1) load(Y + (long long)(n + 2) * frame_stride, A);
            accumulate(interior, B);
        }
    };
    if (y0 >= 1 && y0 + R - 1 <= H - 2) walk(std::true_type{});
    else walk(std::false_type{});

    // flush: lanes 1..62, pixels inside the frame; SM only off the outer ring
    if (lane < 1 || lane > 62 || n0 >= n1) return;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int y = y0 + r;
        if (y >= H) break;
#pragma unroll
        for (int i = 0; i < kLfLaneCols; ++i) {
            const int x = x0 + i;
            if (x >= W) break;
            const long long p = (long long)y * W + x;
            if (s1[r][i]) atomicAdd(&S1[p], (unsigned long long)s1[r][i]);
            if (sm[r][i] && x >= 1 && x <= W - 2) atomicAdd(&SM[p], (unsigned long long)sm[r][i]);     // (columns 0 and W-1: the ring)
        }
    }
}

// logofind_msb_kernels.hip: launch_logofind's batches with b.shift != 0 (bits = the depth of the shifted samples, 9..16; shift = 16 - bits)
struct FrameBatch;
hipError_t launch_logofind_msb(hipStream_t st, int bits, const FrameBatch& b, int W, int H, int nframes, int num_cus, unsigned long long* dS1,
                               unsigned long long* dSM);
// the grid of a launch over nframes frames: tiles x frame slices
struct LfGrid { int col_waves, tiles, slice_frames, slices; bool buf; };
inline LfGrid logofind_grid(int pitch_elems, int W, int H, int nframes, int num_cus)
{
    LfGrid g;
    g.col_waves = (W + kLfSpan - 1) / kLfSpan;
    g.tiles = (H + kLfRows - 1) / kLfRows * g.col_waves;
    // slices: enough waves for ~16 per CU, but no slice shorter than kLfMinSliceFrames frames
    const long long want = ((long long)std::max(1, num_cus) * 16 + g.tiles - 1) / g.tiles;
    const long long most = std::max(1, nframes / kLfMinSliceFrames);
    const int slices = (int)std::max(1LL, std::min(want, most));
    g.slice_frames = (nframes + slices - 1) / slices;
    g.slices = (nframes + g.slice_frames - 1) / g.slice_frames;
    g.buf = (long long)((W + kLfLaneCols - 1) / kLfLaneCols) * kLfLaneCols <= pitch_elems;
    return g;
}

} // namespace amt
