// lane_rule_test.cpp -- the lane-width selections of amatsukaze_amd/csrc/lane_rule.h against the expressions the launchers wrote out by
// hand before there was one rule: every `was_*` below is that launcher's selection as it stood, copied as plain integer arithmetic
// (uintptr_t casts became uint64_t), and each is compared with the function that replaced it over every combination of a small domain.
// Exits non-zero at the first difference, printing the site and the inputs.
//   usage: lane_rule_test          (no arguments; prints the number of combinations per site)
//
// Domain.  Addresses are kBase + offset.  P32: offsets 0..31; P5: {0, 1, 2, 4, 8} (every alignment class a width up to 16 can tell
// apart); S14: {0, 1, 2, 4, 6, 8, 12, 16, 24, 32, 48, 1472, 1474, 2944}; S6: {0, 1, 2, 4, 8, 1474}; W64: 1..64 samples;
// W14: {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 33, 48, 63, 64}; W8: {1, 2, 3, 4, 8, 16, 17, 64}; es 1 and 2 everywhere.
//   scan keep, luma            src P32, store P32, stride S14 (samples, as the old descriptor counted), pitch S14, w W64
//   scan keep, chroma          srcU P32, srcV / storeU / storeV P5, stride S6, pitch S6, wUV W14
//   surfaces extract, luma     src P32, dst P5, source and destination stride and pitch S6 each, w W14
//   surfaces extract, chroma   srcU P32, srcV / dstU / dstV P5, source and destination stride and pitch S6 each, wUV W8, planar and
//                              interleaved (lane bytes and pairC; srcV is null when interleaved, as in the launcher)
//   surface Delogo, luma       src P32, dst P32, stride S14 (bytes), pitch S14 (containers), w W64
//   surface Delogo, chroma     sU P32, sV / U / V P5, stride S6, pitch S6, wUV W64, planar and interleaved
//   Delogo pair, luma          src P32, dst P32, stride S14 (samples), pitch S14, imgx 0..7, w W14
//   Delogo pair, chroma        srcU P32, srcV / dstU / dstV P5, stride S6 (samples), pitch S6, cx 0..3, wUV W14
//   ingest rows                src P32, dst P32, both strides S14, chunk 1..64 bytes
//   render vec                 srcY P32, the other five planes {0, 8}, the four strides and four pitches {0, 8, -16}
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lane_rule.h"

using namespace amt;
typedef uint64_t U;
typedef long long L;
typedef std::vector<L> Set;

static const U kBase = 0x7f3a00001000ull;

// ---- the selections as the launchers wrote them ----
static int was_keep(int es, U src, U src2, U store, U store2, L stride_samples, L pitch_samples, L w)
{
    const L stride = stride_samples * es, pitch = pitch_samples * es, row = w * es;
    auto width = [es](U v) { return v % 16 == 0 ? 16 : v % 4 == 0 ? 4 : es; };
    return width(src | src2 | store | store2 | (U)stride | (U)pitch | (U)row);
}
static bool bits_of(U v, U m) { return v % m == 0; }
static int was_extract(int es, U srcbits, U dstbits) { return bits_of(srcbits | dstbits, 16) ? 16 : bits_of(srcbits | dstbits, 4) ? 4 : es; }
static int was_extract_split(int es, U srcCbits, U dstCbits)
{
    return bits_of(srcCbits, 16) && bits_of(dstCbits, 8) ? 16 : bits_of(srcCbits, 4) && bits_of(dstCbits, 2) ? 4 : 2 * es;
}
static int was_extract_pair(int il, U srcCbits, U dstCbits) { return il && !(bits_of(srcCbits, 4) && bits_of(dstCbits, 2)); }
static int was_delogo_surface(int es, U bits)
{
    auto width = [es](U v) { return v % (4 * (U)es) == 0 ? 4 : v % (2 * (U)es) == 0 ? 2 : 1; };
    return width(bits);
}
static int was_delogo_pair(int es, L w, L origin, L pitch, L stride_samples, U d0, U d1, U s0, U s1)
{
    auto even = [](L v) { return (v & 1) == 0; };
    auto aligned = [&](U p) { return p % (2 * es) == 0; };
    return even(w) && even(origin) && even(pitch) && even(stride_samples) && aligned(d0) && aligned(d1) && aligned(s0) && aligned(s1);
}
static int was_ingest(U src, U dst, L src_stride, L dst_stride, U chunk)
{
    const U a = src | dst | (U)src_stride | (U)dst_stride | chunk;
    return (a % 16 == 0) ? 16 : (a % 4 == 0) ? 4 : 1;
}
static bool al16(U p, L stride, int pitch) { return p % 16 == 0 && stride % 16 == 0 && pitch % 16 == 0; }

// ---- every combination of the sets, odometer order ----
static long long g_count = 0;
template <typename F> static void for_all(const char* site, const std::vector<Set>& sets, F&& differs)
{
    const size_t n = sets.size();
    std::vector<size_t> at(n, 0);
    std::vector<L> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = sets[i][0];
    long long count = 0;
    for (;;) {
        ++count;
        int was = 0, is = 0;
        if (differs(v.data(), was, is)) {
            fprintf(stderr, "FAIL %s: was %d, lane_rule.h gives %d for inputs", site, was, is);
            for (size_t i = 0; i < n; ++i) fprintf(stderr, " %lld", v[i]);
            fprintf(stderr, "\n");
            exit(1);
        }
        size_t k = 0;
        while (k < n && ++at[k] == sets[k].size()) { at[k] = 0; v[k] = sets[k][0]; ++k; }
        if (k == n) break;
        v[k] = sets[k][at[k]];
    }
    printf("%-28s %12lld combinations\n", site, count);
    g_count += count;
}
static Set range(L lo, L hi) { Set s; for (L i = lo; i <= hi; ++i) s.push_back(i); return s; }

int main()
{
    const Set P32 = range(0, 31), P5 = {0, 1, 2, 4, 8}, S14 = {0, 1, 2, 4, 6, 8, 12, 16, 24, 32, 48, 1472, 1474, 2944}, S6 = {0, 1, 2, 4, 8, 1474};
    const Set W64 = range(1, 64), W14 = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 33, 48, 63, 64}, W8 = {1, 2, 3, 4, 8, 16, 17, 64}, ES = {1, 2}, ONOFF = {0, 1};
    auto A = [](L off) { return kBase + (U)off; };

    for_all("scan keep luma", {ES, P32, P32, S14, S14, W64}, [&](const L* v, int& was, int& is) {
        const int es = (int)v[0];
        was = was_keep(es, A(v[1]), 0, A(v[2]), 0, v[3], v[4], v[5]);
        is = scan_keep_lane_bytes(es, RowsAt{A(v[1]), 0, v[3] * es, v[4] * es}, A(v[2]), 0, v[5] * es);
        return was != is;
    });
    for_all("scan keep chroma", {ES, P32, P5, P5, P5, S6, S6, W14}, [&](const L* v, int& was, int& is) {
        const int es = (int)v[0];
        was = was_keep(es, A(v[1]), A(v[2]), A(v[3]), A(v[4]), v[5], v[6], v[7]);
        is = scan_keep_lane_bytes(es, RowsAt{A(v[1]), A(v[2]), v[5] * es, v[6] * es}, A(v[3]), A(v[4]), v[7] * es);
        return was != is;
    });
    for_all("surfaces extract luma", {ES, P32, P5, S6, S6, S6, S6, W14}, [&](const L* v, int& was, int& is) {
        const int es = (int)v[0];
        const L spitch = v[4] * es, dpitch = v[6] * es, row = v[7] * es;
        was = was_extract(es, A(v[1]) | (U)v[3] | (U)spitch | (U)row, A(v[2]) | (U)v[5] | (U)dpitch);
        is = extract_lane_bytes(es, RowsAt{A(v[1]), 0, v[3], spitch}, RowsAt{A(v[2]), 0, v[5], dpitch}, row);
        return was != is;
    });
    for_all("surfaces extract chroma", {ES, ONOFF, P32, P5, P5, P5, S6, S6, S6, S6, W8}, [&](const L* v, int& was, int& is) {
        const int es = (int)v[0], il = (int)v[1];
        const U srcU = A(v[2]), srcV = il ? 0 : A(v[3]), dstU = A(v[4]), dstV = A(v[5]);
        const L spitch = v[7] * es, dpitch = v[9] * es, row = v[10] * es * (il ? 2 : 1);
        const U srcCbits = srcU | srcV | (U)v[6] | (U)spitch | (U)row, dstCbits = dstU | dstV | (U)v[8] | (U)dpitch;
        const RowsAt srcC{srcU, srcV, v[6], spitch}, dstC{dstU, dstV, v[8], dpitch};
        const SplitLanes split = extract_split_lanes(es, srcC, dstC, row);
        // lane bytes and pairC in one number, as the launcher now forms them
        was = (il ? was_extract_split(es, srcCbits, dstCbits) : was_extract(es, srcCbits, dstCbits)) * 2 + was_extract_pair(il, srcCbits, dstCbits);
        is = (il ? split.bytes : extract_lane_bytes(es, srcC, dstC, row)) * 2 + (il ? split.pairwise : 0);
        return was != is;
    });
    for_all("surface Delogo luma", {ES, P32, P32, S14, S14, W64}, [&](const L* v, int& was, int& is) {
        const int es = (int)v[0];
        was = was_delogo_surface(es, A(v[1]) | A(v[2]) | (U)v[3] | (U)(v[4] * es) | (U)(v[5] * es));
        is = delogo_surface_lane_containers(es, RowsAt{A(v[1]), 0, v[3], v[4] * es}, RowsAt{A(v[2]), 0, v[3], v[4] * es}, v[5] * es);
        return was != is;
    });
    for_all("surface Delogo chroma", {ES, ONOFF, P32, P5, P5, P5, S6, S6, W64}, [&](const L* v, int& was, int& is) {
        const int es = (int)v[0], il = (int)v[1];
        const U sU = A(v[2]), sV = il ? 0 : A(v[3]), dU = A(v[4]), dV = il ? 0 : A(v[5]);
        const L pitch = v[7] * es, row = (il ? 2LL : 1LL) * v[8] * es;
        was = was_delogo_surface(es, sU | sV | dU | dV | (U)v[6] | (U)pitch | (U)row);
        is = delogo_surface_lane_containers(es, RowsAt{sU, sV, v[6], pitch}, RowsAt{dU, dV, v[6], pitch}, row);
        return was != is;
    });
    for_all("Delogo pair luma", {ES, P32, P32, S14, S14, range(0, 7), W14}, [&](const L* v, int& was, int& is) {
        const int es = (int)v[0];
        was = was_delogo_pair(es, v[6], v[5], v[4], v[3], A(v[2]), 0, A(v[1]), 0);
        is = delogo_pair_lanes(es, RowsAt{A(v[1]), 0, v[3] * es, v[4] * es}, RowsAt{A(v[2]), 0, v[3] * es, v[4] * es}, v[5] * es, v[6] * es);
        return was != is;
    });
    for_all("Delogo pair chroma", {ES, P32, P5, P5, P5, S6, S6, range(0, 3), W14}, [&](const L* v, int& was, int& is) {
        const int es = (int)v[0];
        was = was_delogo_pair(es, v[8], v[7], v[6], v[5], A(v[3]), A(v[4]), A(v[1]), A(v[2]));
        is = delogo_pair_lanes(es, RowsAt{A(v[1]), A(v[2]), v[5] * es, v[6] * es}, RowsAt{A(v[3]), A(v[4]), v[5] * es, v[6] * es}, v[7] * es, v[8] * es);
        return was != is;
    });
    for_all("ingest rows", {P32, P32, S14, S14, range(1, 64)}, [&](const L* v, int& was, int& is) {
        was = was_ingest(A(v[0]), A(v[1]), v[2], v[3], (U)v[4]);
        is = ingest_lane_bytes(A(v[0]), A(v[1]), v[2], v[3], (unsigned long long)v[4]);
        return was != is;
    });
    const Set P2 = {0, 8}, T3 = {0, 8, -16};
    for_all("render vec", {P32, P2, P2, P2, P2, P2, T3, T3, T3, T3, T3, T3, T3, T3}, [&](const L* v, int& was, int& is) {
        const U srcY = A(v[0]), srcU = A(v[1]), srcV = A(v[2]), dstY = A(v[3]), dstU = A(v[4]), dstV = A(v[5]);
        const L sstrideY = v[6], sstrideUV = v[7], dstrideY = v[8], dstrideUV = v[9];
        const int spitchY = (int)v[10], spitchUV = (int)v[11], dpitchY = (int)v[12], dpitchUV = (int)v[13];
        was = al16(srcY, sstrideY, spitchY) && al16(srcU, sstrideUV, spitchUV) && al16(srcV, sstrideUV, spitchUV) && al16(dstY, dstrideY, dpitchY) &&
              al16(dstU, dstrideUV, dpitchUV) && al16(dstV, dstrideUV, dpitchUV);
        is = render_vec16(RowsAt{srcY, 0, sstrideY, spitchY}, RowsAt{srcU, srcV, sstrideUV, spitchUV}, RowsAt{dstY, 0, dstrideY, dpitchY},
                          RowsAt{dstU, dstV, dstrideUV, dpitchUV});
        return was != is;
    });
    printf("%lld combinations, no difference\n", g_count);
    return 0;
}
