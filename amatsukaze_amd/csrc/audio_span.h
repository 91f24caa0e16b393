// audio_span.h -- how audio_levels_kernel (audio_kernels.hip) cuts one video frame's PCM span into head, body and tail, and which bytes
// each lane loads: the address arithmetic behind "no load touches a byte outside the span", as pure functions of integers.  The kernel
// calls these functions; tests/cpp/audio_span_replay.cpp compiles this file with plain g++ and replays every load of a grid of spans on
// the host.  No HIP in this file.
//
// A span is the elements [e0, e1) of the int16 array at `pcm` (e1 > e0: an empty span is never split and addresses nothing); every
// offset below is in BYTES from `pcm`, whose low four address bits are `mis` (even: the pointer is aligned to 2 bytes).
//   head  [a0, b0): the elements before the first 16-byte boundary inside the span (at most 7; all of a span that holds no boundary)
//   body  [b0, b1): nchunks aligned 16-byte chunks, read in groups of 64 * kAudioGroup: slot k of a lane is chunk c0 + 64 * k + lane
//   tail  [b1, a1): the elements behind the last boundary (at most 7)
// The structs travel BY VALUE and `counts` is formed from head and tail where it is used: that way the kernel compiles to the
// instructions it had when these expressions stood in its body (by reference, or with the predicate folded into the load's struct, the
// compiler orders the loop's registers differently).
#pragma once

namespace amt {

#if defined(__HIPCC__)
#define AMT_SPAN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define AMT_SPAN_HD inline
#endif

constexpr int kAudioGroup = 8;                        // 16-byte loads a lane has in flight

struct AudioSpan {
    long long a0, a1;                                 // the span
    long long b0, b1;                                 // its body
    unsigned nhead, ntail;                            // elements in front of and behind the body
    long long nchunks;
};

AMT_SPAN_HD long long audio_span_min(long long a, long long b) { return a < b ? a : b; }
AMT_SPAN_HD long long audio_span_max(long long a, long long b) { return a > b ? a : b; }

AMT_SPAN_HD AudioSpan audio_span_split(unsigned mis, long long e0, long long e1)
{
    AudioSpan s;
    s.a0 = 2 * e0, s.a1 = 2 * e1;
    s.b0 = audio_span_min(((s.a0 + mis + 15) & ~15LL) - mis, s.a1);       // the span's start rounded UP to a 16-byte address, at most its end
    s.b1 = audio_span_max(((s.a1 + mis) & ~15LL) - mis, s.b0);            // its end rounded DOWN, never below b0
    s.nhead = (unsigned)(s.b0 - s.a0) / 2, s.ntail = (unsigned)(s.a1 - s.b1) / 2;
    s.nchunks = (s.b1 - s.b0) / 16;
    return s;
}

// One lane's 16-byte load of slot k (0 .. kAudioGroup - 1) of the group that starts at chunk c0 < nchunks.  A lane of the last group that
// has no chunk re-reads the span's last one (`mine` is false: the value is dropped).
// The kernel indexes 16-byte vectors from pcm + b0 with `chunk`; `off` is that address as a byte offset from pcm.
struct AudioBodyLoad { long long chunk, off; bool mine; };
AMT_SPAN_HD AudioBodyLoad audio_span_body_load(const AudioSpan s, long long c0, int k, unsigned lane)
{
    const long long c = c0 + k * 64 + lane, chunk = audio_span_min(c, s.nchunks - 1);
    return AudioBodyLoad{chunk, s.b0 + 16 * chunk, c < s.nchunks};
}

// One lane's 2-byte load: lanes 0..6 take the head, lanes 8..14 the tail; a lane without an element reads the span's first one (it
// exists) and drops it (audio_span_edge_counts is false).
struct AudioEdgeLoad { long long off; bool head, tail; };
AMT_SPAN_HD bool audio_span_edge_counts(const AudioEdgeLoad e) { return e.head || e.tail; }
AMT_SPAN_HD AudioEdgeLoad audio_span_edge_load(const AudioSpan s, unsigned lane)
{
    const bool head = lane < s.nhead, tail = lane >= 8 && lane - 8 < s.ntail;
    return AudioEdgeLoad{head ? s.a0 + 2 * lane : tail ? s.b1 + 2 * (lane - 8) : s.a0, head, tail};
}

} // namespace amt
