// audio_span_replay.cpp -- every load of audio_levels_kernel replayed on the host, from the functions the kernel itself calls
// (amatsukaze_amd/csrc/audio_span.h): the split of a span into head, body and tail, the 16-byte body loads of every (group, slot, lane)
// with their clamp, and the 2-byte head / tail load of every lane.  Exits non-zero at the first span that breaks a rule below, printing
// the rule and (mis, e0, e1) -- plus (c0, k, lane) where a single load is at fault.
//   usage: audio_span_replay          (no arguments; prints what the grid reached)
//
// Grid: every even mis in 0..14 (the pointer's low four bits) x every span start e0 in 0..15 x every length 0..8300 elements (just past
// 1025 chunks), and the lengths 8 * n + d, d in 0..8, for n = 11776, 11777, 12000, 12288 (24 groups: the emptiest, one chunk more, the
// 48 kHz stereo second, the full one) and n = 12289, 12800 (25 groups: one chunk in the last, the full one).
//
// Rules, for a span [e0, e1) with e1 > e0, a0 = 2 * e0, a1 = 2 * e1 (bytes from pcm):
//   partition   a0 <= b0 <= b1 <= a1; nhead = (b0 - a0) / 2 <= 7; ntail = (a1 - b1) / 2 <= 7; nchunks * 16 == b1 - b0
//   alignment   b0 + mis and b1 + mis are multiples of 16 -- unless the span holds no 16-byte boundary: then b0 == b1 == a1, the head
//               takes the whole span and there is no aligned address to speak of
//   in bounds   every byte of every load lies in [a0, a1): the 16 bytes of a body load (clamped re-reads included; they lie in
//               [b0, b1) and at a 16-byte address), the 2 bytes of a head or tail load and of the first element an idle lane reads
//   once        every body chunk is `mine` for exactly one (group, slot, lane); every head and every tail element counts for exactly
//               one lane, and no body element does
// The kernel addresses a body load as a 16-byte vector index `chunk` from pcm + b0: off == b0 + 16 * chunk is checked with it.
// An empty span (e1 == e0) is behind the kernel's `if (s1 > s0)`: replay() has the same guard and must issue no load for it; the split
// of an empty span, were it made, has no head, no tail and no chunk.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "audio_span.h"

using namespace amt;
typedef long long L;

static unsigned g_mis;
static L g_e0, g_e1;
static void fail(const char* rule)
{
    fprintf(stderr, "FAIL %s: mis %u, e0 %lld, e1 %lld\n", rule, g_mis, g_e0, g_e1);
    exit(1);
}
static void fail_load(const char* rule, L c0, int k, unsigned lane)
{
    fprintf(stderr, "FAIL %s: mis %u, e0 %lld, e1 %lld, group at chunk %lld, slot %d, lane %u\n", rule, g_mis, g_e0, g_e1, c0, k, lane);
    exit(1);
}

struct Reached {
    L spans = 0, loads = 0, max_groups = 0, whole_head = 0, empty = 0;
    bool nhead0[8] = {}, ntail0[8] = {};      // head and tail sizes seen with nchunks == 0
    bool groups[32] = {};
    bool last_group_one = false;
};
static Reached R;
static std::vector<int> chunk_hits;

// the kernel's body from `if (s1 > s0)` on, loads replaced by checks; returns the loads issued
static L replay(unsigned mis, L e0, L e1)
{
    L loads = 0;
    if (e1 > e0) {
        const AudioSpan s = audio_span_split(mis, e0, e1);
        const L a0 = 2 * e0, a1 = 2 * e1;
        if (s.a0 != a0 || s.a1 != a1) fail("a0 == 2 * e0 and a1 == 2 * e1");
        if (!(a0 <= s.b0 && s.b0 <= s.b1 && s.b1 <= a1)) fail("a0 <= b0 <= b1 <= a1");
        if ((s.b0 - a0) % 2 || (a1 - s.b1) % 2) fail("head and tail hold whole elements");
        if ((L)s.nhead * 2 != s.b0 - a0 || (L)s.ntail * 2 != a1 - s.b1) fail("head, body and tail partition [a0, a1)");
        if (s.nhead > 7 || s.ntail > 7) fail("nhead <= 7 and ntail <= 7");
        if (s.nchunks < 0 || s.nchunks * 16 != s.b1 - s.b0) fail("nchunks * 16 == b1 - b0");
        const bool aligned = (s.b0 + mis) % 16 == 0 && (s.b1 + mis) % 16 == 0;
        const bool whole_head = s.b0 == a1 && s.b1 == a1 && (a0 + mis + 15) / 16 * 16 > a1 + mis;
        if (!aligned && !whole_head) fail("b0 + mis and b1 + mis are multiples of 16 (or the span holds no boundary and the head takes it whole)");

        chunk_hits.assign((size_t)s.nchunks, 0);
        int edge_hits[16] = {};                   // head elements 0..6 at [0, 7), tail elements at [8, 15)
        for (unsigned lane = 0; lane < 64; ++lane) {
            const AudioEdgeLoad el = audio_span_edge_load(s, lane);
            ++loads;
            if (el.off < a0 || el.off + 2 > a1) fail_load("a head / tail / idle 2-byte load lies in [a0, a1)", -1, -1, lane);
            if ((el.off - a0) % 2) fail_load("a 2-byte load is at an element", -1, -1, lane);
            if (audio_span_edge_counts(el)) {
                if (el.off >= s.b0 && el.off < s.b1) fail_load("no body element counts as head or tail", -1, -1, lane);
                ++edge_hits[el.off < s.b0 ? (el.off - a0) / 2 : 8 + (el.off - s.b1) / 2];      // (inside [a0, a1): below 7 + 1 elements either way)
            }
        }
        for (unsigned n = 0; n < 8; ++n)
            if (edge_hits[n] != (n < s.nhead ? 1 : 0) || edge_hits[8 + n] != (n < s.ntail ? 1 : 0))
                fail("every head and every tail element counts for exactly one lane");
        L groups = 0;
        for (L c0 = 0; c0 < s.nchunks; c0 += 64 * kAudioGroup) {
            ++groups;
            for (int k = 0; k < kAudioGroup; ++k)
                for (unsigned lane = 0; lane < 64; ++lane) {
                    const AudioBodyLoad bl = audio_span_body_load(s, c0, k, lane);
                    ++loads;
                    if (bl.off != s.b0 + 16 * bl.chunk) fail_load("off == b0 + 16 * chunk", c0, k, lane);
                    if (bl.off < s.b0 || bl.off + 16 > s.b1) fail_load("a 16-byte body load lies in [b0, b1)", c0, k, lane);
                    if (bl.off < a0 || bl.off + 16 > a1) fail_load("a 16-byte body load lies in [a0, a1)", c0, k, lane);
                    if ((bl.off + mis) % 16) fail_load("a 16-byte body load is at a 16-byte address", c0, k, lane);
                    if (bl.mine) ++chunk_hits[(size_t)bl.chunk];
                }
        }
        for (L c = 0; c < s.nchunks; ++c)
            if (chunk_hits[(size_t)c] != 1) fail("every body chunk is mine for exactly one (group, slot, lane)");

        if (s.nchunks == 0) R.nhead0[s.nhead] = R.ntail0[s.ntail] = true;
        if (whole_head) ++R.whole_head;
        if (groups < 32) R.groups[groups] = true;
        if (groups > R.max_groups) R.max_groups = groups;
        if (s.nchunks % (64 * kAudioGroup) == 1) R.last_group_one = true;
    }
    return loads;
}

static void one(unsigned mis, L e0, L len)
{
    g_mis = mis, g_e0 = e0, g_e1 = e0 + len;
    const L loads = replay(mis, e0, e0 + len);
    ++R.spans;
    R.loads += loads;
    if (len == 0) {
        ++R.empty;
        if (loads != 0) fail("an empty span issues no load");
        const AudioSpan s = audio_span_split(mis, e0, e0);
        if (s.nhead || s.ntail || s.nchunks) fail("an empty span has no head, no tail and no chunk");
    }
}

int main()
{
    std::vector<L> lengths;
    for (L len = 0; len <= 8300; ++len) lengths.push_back(len);
    for (L n : {11776LL, 11777LL, 12000LL, 12288LL, 12289LL, 12800LL})
        for (L d = 0; d <= 8; ++d) lengths.push_back(8 * n + d);
    for (unsigned mis = 0; mis < 16; mis += 2)
        for (L e0 = 0; e0 < 16; ++e0)
            for (L len : lengths) one(mis, e0, len);

    // what the grid reached (a grid that stopped reaching these would check less than it says)
    g_mis = 0, g_e0 = g_e1 = 0;
    for (int n = 0; n <= 7; ++n)
        if (!R.nhead0[n] || !R.ntail0[n]) fail("the grid holds every head and tail size 0..7 with zero chunks");
    for (int g : {0, 1, 2, 3, 24, 25})
        if (!R.groups[g]) fail("the grid holds spans of 0, 1, 2, 3, 24 and 25 groups");
    if (!R.whole_head || !R.last_group_one || !R.empty) fail("the grid holds whole-head spans, last groups of one chunk and empty spans");
    printf("%lld spans (%lld empty, %lld taken whole by the head), %lld loads, up to %lld groups: every rule holds\n", R.spans, R.empty,
           R.whole_head, R.loads, R.max_groups);
    return 0;
}
