// audio_kernels.hip -- per-video-frame audio levels (self-specified): one read-once pass over interleaved
// little-endian int16 PCM that leaves, per video frame, {max |s|, sum |s|, sum s*s, elements} of the sample-frames the frame owns.
//
// Video frame n owns sample-frames [b(n), b(n + 1)) with b(n) = floor(n * sample_rate * fps_den / fps_num), cut at num_samples.  One
// wave takes one video frame, four frames share a 256-thread workgroup (nothing is shared between them: no LDS, no barrier).  A span
// is about 6.4 KB at 48 kHz stereo and 29.97 fps and starts on any even byte, so a wave splits it into
//   head  the elements before the first 16-byte boundary inside the span (at most 7; all of a span that holds no boundary),
//   body  whole 16-byte chunks, chunk c of a group of 512 to lane c % 64: non-temporal dwordx4 loads from aligned addresses, the up to
//         8 of a lane all issued before the first is used (7 at 48 kHz stereo: one group),
//   tail  the elements behind the last boundary (at most 7),
// head and tail read with one 2-byte load per lane (lanes 0..6 and 8..14).  The aligned addresses are found by rounding the span's START
// UP and its END DOWN, so no load touches a byte outside the span, let alone outside the caller's buffer.  A lane of the last group that
// has no chunk re-reads the span's last one and drops the value (branch-free: the loads of a group leave back to back).  The split
// and the offset of every load are audio_span.h's functions, which tests/cpp/audio_span_replay.cpp replays on the host.
//
// Exact for every input: |s| is taken in packed 16-bit lanes as max(s, 0 - s), which leaves 0x8000 for -32768 -- 32768 once the lane is
// read as UNSIGNED, as every later step does; the sum of |s| is kept in 32 bits for one group (64 elements a lane: at most 2^21) and in
// 64 bits across groups; a squared sample is up to 2^30, two of them (one dword) fill 32 bits exactly, and every dword's pair is added
// to a 64-bit total.  The wave's 64 partials are folded by DPP (row_shr / row_bcast, stats_body.h's pattern; the 64-bit sums as two
// halves moved by the same DPP control and one 64-bit add per step) into lane 63, which writes the record with plain stores.
#include "build_knobs.h"
#include "audio_span.h"
#include "kernels.hpp"

#include <hip/hip_runtime.h>
#include <cstdint>

namespace amt {
namespace {

constexpr int kAudioThreads = 256;
constexpr int kAudioWaves = kAudioThreads / 64;       // video frames per workgroup

typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef short s2 __attribute__((ext_vector_type(2)));
typedef unsigned short us2 __attribute__((ext_vector_type(2)));

// what one lane has seen so far
struct AudioAcc {
    us2 peak = {0, 0};
    unsigned sumabs32 = 0;                            // of the current group, folded into sumabs by fold()
    unsigned long long sumabs = 0, sumsq = 0;
    // two samples in one dword
    __device__ __forceinline__ void add(unsigned w)
    {
        const us2 u = __builtin_bit_cast(us2, w);
        const us2 neg = (us2)(0) - u;                 // (unsigned: wraps, 0 - 0x8000 = 0x8000)
        const us2 a = __builtin_bit_cast(us2, __builtin_elementwise_max(__builtin_bit_cast(s2, u), __builtin_bit_cast(s2, neg)));
        peak = __builtin_elementwise_max(peak, a);
        sumabs32 = __builtin_amdgcn_sad_u16(__builtin_bit_cast(unsigned, a), 0u, sumabs32);
        sumsq += (unsigned)a.x * (unsigned)a.x + (unsigned)a.y * (unsigned)a.y;      // <= 2^31: fits 32 bits before it is widened
    }
    __device__ __forceinline__ void fold() { sumabs += sumabs32; sumabs32 = 0; }
};

template <int CTRL, int ROW_MASK> __device__ __forceinline__ unsigned dpp_from(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);      // lanes without a source get 0
}
// max / sum over the 64 lanes of a wave, result in lane 63 (wave_sum_to_lane63's steps, stats_body.h)
__device__ __forceinline__ unsigned wave_max_to_lane63(unsigned v)
{
    v = max(v, dpp_from<0x111, 0xF>(v));
    v = max(v, dpp_from<0x112, 0xF>(v));
    v = max(v, dpp_from<0x114, 0xF>(v));
    v = max(v, dpp_from<0x118, 0xF>(v));
    v = max(v, dpp_from<0x142, 0xA>(v));
    v = max(v, dpp_from<0x143, 0xC>(v));
    return v;
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ unsigned long long dpp_from64(unsigned long long v)
{
    return ((unsigned long long)dpp_from<CTRL, ROW_MASK>((unsigned)(v >> 32)) << 32) | dpp_from<CTRL, ROW_MASK>((unsigned)v);
}
__device__ __forceinline__ unsigned long long wave_sum64_to_lane63(unsigned long long v)
{
    v += dpp_from64<0x111, 0xF>(v);
    v += dpp_from64<0x112, 0xF>(v);
    v += dpp_from64<0x114, 0xF>(v);
    v += dpp_from64<0x118, 0xF>(v);
    v += dpp_from64<0x142, 0xA>(v);
    v += dpp_from64<0x143, 0xC>(v);
    return v;
}
__device__ __forceinline__ unsigned long long read_lane64(unsigned long long v, int lane)
{
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(v >> 32), lane) << 32) |
           (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
}

__global__ __launch_bounds__(kAudioThreads)
void audio_levels_kernel(const int16_t* __restrict__ pcm, long long pcm_first, AudioTimeline t, long long first_frame, int nframes,
                         unsigned long long* __restrict__ out)
{
    const unsigned lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long i = (long long)blockIdx.x * kAudioWaves + wave;          // the batch's frame of this wave
    if (i >= nframes) return;

    // b(n) in lane 0 and b(n + 1) in lane 1: one 64-bit division per wave (the host has checked that the product fits)
    unsigned long long edge = (unsigned long long)(first_frame + i + (lane & 1)) * (unsigned long long)t.step_num / (unsigned long long)t.fps_num;
    edge = min(edge, (unsigned long long)t.num_samples);
    const long long s0 = (long long)read_lane64(edge, 0), s1 = (long long)read_lane64(edge, 1);
    AudioAcc acc;
    long long count = 0;
    // an empty span (all of the frame behind the timeline) need not lie inside the caller's range: nothing of it is addressed
    if (s1 > s0) {
        const long long e0 = (s0 - pcm_first) * t.channels, e1 = (s1 - pcm_first) * t.channels;      // elements of pcm
        count = e1 - e0;
        // byte offsets from pcm (every address below is pcm + offset: the loads stay global ones); the split and every offset: audio_span.h
        const AudioSpan sp = audio_span_split((unsigned)(uintptr_t)pcm & 15u, e0, e1);
        const char* const bytes = reinterpret_cast<const char*>(pcm);

        // head and tail: lanes without an element read the span's first one (it exists) and drop it
        const AudioEdgeLoad edge_load = audio_span_edge_load(sp, lane);
        const unsigned edge_word = *reinterpret_cast<const unsigned short*>(bytes + edge_load.off);

        const u4* body = reinterpret_cast<const u4*>(bytes + sp.b0);
        for (long long c0 = 0; c0 < sp.nchunks; c0 += 64 * kAudioGroup) {
            u4 v[kAudioGroup];
#pragma unroll
            for (int k = 0; k < kAudioGroup; ++k)
                v[k] = __builtin_nontemporal_load(body + audio_span_body_load(sp, c0, k, lane).chunk);
            __builtin_amdgcn_sched_barrier(0);            // the group's loads all leave before the first value is used
#pragma unroll
            for (int k = 0; k < kAudioGroup; ++k) {
                const bool mine = audio_span_body_load(sp, c0, k, lane).mine;
#pragma unroll
                for (int j = 0; j < 4; ++j) acc.add(mine ? v[k][j] : 0u);
            }
            acc.fold();
        }
        acc.add(audio_span_edge_counts(edge_load) ? edge_word : 0u);
        acc.fold();
    }

    const unsigned peak = wave_max_to_lane63(max((unsigned)acc.peak.x, (unsigned)acc.peak.y));
    const unsigned long long sumabs = wave_sum64_to_lane63(acc.sumabs), sumsq = wave_sum64_to_lane63(acc.sumsq);
    if (lane == 63) {
        unsigned long long* rec = out + i * kAudioLevelWords;
        rec[0] = peak;
        rec[1] = sumabs;
        rec[2] = sumsq;
        rec[3] = (unsigned long long)count;
    }
}

} // namespace

hipError_t launch_audio_levels(hipStream_t st, const int16_t* dpcm, long long pcm_first, const AudioTimeline& t, long long first_frame,
                               int nframes, unsigned long long* dout)
{
    if (nframes <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((nframes + kAudioWaves - 1) / kAudioWaves);
    hipLaunchKernelGGL(audio_levels_kernel, dim3(grid), dim3(kAudioThreads), 0, st, dpcm, pcm_first, t, first_frame, nframes, dout);
    return hipGetLastError();
}

} // namespace amt
