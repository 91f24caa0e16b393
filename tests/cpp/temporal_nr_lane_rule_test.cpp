// temporal_nr_lane_rule_test.cpp -- temporal_nr_vec16 (amatsukaze_amd/csrc/lane_rule.h) against a brute-force check: the vector form of
// temporal_nr_kernel makes 16-byte accesses at luma rows and 8-byte accesses at chroma rows, so the selection must be 1 exactly where
// every row start base + n * stride + y * pitch (n, y in 0..1) of every luma plane is a multiple of 16 and of every chroma plane a
// multiple of 8.  Exits non-zero at the first difference, printing the inputs.
//   usage: temporal_nr_lane_rule_test          (no arguments; prints the number of combinations)
//
// Domain: srcY at offsets {0, 1, 2, 4, 8, 16, 24} from a page-aligned base, dstY at {0, 8, 16}, the four chroma planes at {0, 4, 8}; luma strides and
// pitches {0, 8, 16, -16}, chroma strides and pitches {0, 4, 8}.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lane_rule.h"

using namespace amt;
typedef uint64_t U;
typedef long long L;

static const U kBase = 0x7f3a00001000ull;

static bool rows_aligned(U base, L stride, L pitch, U width)
{
    for (int n = 0; n < 2; ++n)
        for (int y = 0; y < 2; ++y)
            if ((base + (U)(n * stride) + (U)(y * pitch)) % width) return false;
    return true;
}

int main()
{
    const std::vector<L> srcYOff = {0, 1, 2, 4, 8, 16, 24}, lumaOff = {0, 8, 16}, chromaOff = {0, 4, 8}, lumaStep = {0, 8, 16, -16}, chromaStep = {0, 4, 8};
    long long count = 0;
    for (L sy : srcYOff)
    for (L dy : lumaOff) for (L su : chromaOff) for (L sv : chromaOff) for (L du : chromaOff) for (L dv : chromaOff)
    for (L ssY : lumaStep) for (L spY : lumaStep) for (L dsY : lumaStep) for (L dpY : lumaStep)
    for (L ssC : chromaStep) for (L spC : chromaStep) for (L dsC : chromaStep) for (L dpC : chromaStep) {
        const U srcY = kBase + (U)sy, dstY = kBase + (U)dy, srcU = kBase + (U)su, srcV = kBase + (U)sv, dstU = kBase + (U)du, dstV = kBase + (U)dv;
        const int want = rows_aligned(srcY, ssY, spY, 16) && rows_aligned(dstY, dsY, dpY, 16) && rows_aligned(srcU, ssC, spC, 8) &&
                         rows_aligned(srcV, ssC, spC, 8) && rows_aligned(dstU, dsC, dpC, 8) && rows_aligned(dstV, dsC, dpC, 8);
        const int is = temporal_nr_vec16(RowsAt{srcY, 0, ssY, spY}, RowsAt{srcU, srcV, ssC, spC}, RowsAt{dstY, 0, dsY, dpY}, RowsAt{dstU, dstV, dsC, dpC});
        ++count;
        if (want != is) {
            fprintf(stderr, "FAIL temporal nr vec: brute force %d, lane_rule.h gives %d for inputs %lld %lld %lld %lld %lld %lld | %lld %lld %lld %lld | %lld %lld %lld %lld\n",
                    want, is, sy, dy, su, sv, du, dv, ssY, spY, dsY, dpY, ssC, spC, dsC, dpC);
            return 1;
        }
    }
    printf("temporal nr vec %lld combinations, no difference\n", count);
    return 0;
}
