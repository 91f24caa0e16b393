// resize_lane_rule_test.cpp -- resize_vec16 (amatsukaze_amd/csrc/lane_rule.h) against a brute-force check: the vector forms of the resize
// kernels make 16-byte accesses at rows of the source, the intermediate and the destination, luma and chroma alike, so the selection
// must be 1 exactly where every row start base + n * stride + y * pitch (n, y in 0..1) of all nine planes is a multiple of 16.
// Exits non-zero at the first difference, printing the inputs.
//   usage: resize_lane_rule_test          (no arguments; prints the number of combinations)
//
// Domain: source and destination planes at offsets {0, 1, 2, 8, 16} (luma) and {0, 8, 16} (each chroma plane) from a page-aligned base,
// the intermediate's at {0, 16, 8}; strides and pitches {0, 8, 16, 48, -16} for the source and the destination, {16, 8} for the
// intermediate.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lane_rule.h"

using namespace amt;
typedef uint64_t U;
typedef long long L;

static const U kBase = 0x7f3a00001000ull;

static bool rows_aligned(U base, L stride, L pitch)
{
    for (int n = 0; n < 2; ++n)
        for (int y = 0; y < 2; ++y)
            if ((base + (U)(n * stride) + (U)(y * pitch)) % 16) return false;
    return true;
}

int main()
{
    const std::vector<L> lumaOff = {0, 1, 2, 8, 16}, chromaOff = {0, 8, 16}, midOff = {0, 16, 8}, step = {0, 8, 16, 48, -16}, midStep = {16, 8};
    long long count = 0, ones = 0;
    for (L sy : lumaOff) for (L dy : lumaOff) for (L su : chromaOff) for (L sv : chromaOff) for (L du : chromaOff) for (L dv : chromaOff)
    for (L my : midOff) for (L mc : midOff)
    for (L ssY : step) for (L spY : step) for (L dsC : step) for (L dpC : step)
    for (L msY : midStep) for (L mpC : midStep) {
        // (source luma and destination chroma take the full step domain; the other two of each kind take a fixed aligned step)
        const RowsAt srcY{kBase + (U)sy, 0, ssY, spY}, srcUV{kBase + (U)su, kBase + (U)sv, 32, 16}, midY{kBase + (U)my, 0, msY, 16},
                     midUV{kBase + (U)mc, kBase + (U)mc + 64, 32, mpC}, dstY{kBase + (U)dy, 0, 64, 32}, dstUV{kBase + (U)du, kBase + (U)dv, dsC, dpC};
        const int want = rows_aligned(srcY.base, ssY, spY) && rows_aligned(srcUV.base, 32, 16) && rows_aligned(srcUV.base2, 32, 16) &&
                         rows_aligned(midY.base, msY, 16) && rows_aligned(midUV.base, 32, mpC) && rows_aligned(midUV.base2, 32, mpC) &&
                         rows_aligned(dstY.base, 64, 32) && rows_aligned(dstUV.base, dsC, dpC) && rows_aligned(dstUV.base2, dsC, dpC);
        const int is = resize_vec16(srcY, srcUV, midY, midUV, dstY, dstUV);
        ++count;
        ones += is;
        if (want != is) {
            fprintf(stderr, "FAIL resize vec: brute force %d, lane_rule.h gives %d for inputs %lld %lld %lld %lld %lld %lld | %lld %lld | %lld %lld %lld %lld | %lld %lld\n",
                    want, is, sy, dy, su, sv, du, dv, my, mc, ssY, spY, dsC, dpC, msY, mpC);
            return 1;
        }
    }
    if (!ones || ones == count) { fprintf(stderr, "FAIL resize vec: the domain holds only one answer\n"); return 1; }
    printf("resize vec %lld combinations (%lld vector), no difference\n", count, ones);
    return 0;
}
