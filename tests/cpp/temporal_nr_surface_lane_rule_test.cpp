// temporal_nr_surface_lane_rule_test.cpp -- temporal_nr_surface_vec16 (amatsukaze_amd/csrc/lane_rule.h) against a brute-force check: the
// vector forms of temporal_nr_surfaces_kernel make 16-byte accesses at luma rows and, at chroma rows, ONE 16-byte access at the UV row
// when interleaved and 8-byte accesses at the U and the V row when planar.  So the selection must be 1 exactly where every row start
// base + n * stride + y * pitch (n, y in 0..1) of every luma plane is a multiple of 16 and of every chroma plane a multiple of 16
// (interleaved; there is no second chroma plane: its base is 0) or 8 (planar).  Exits non-zero at the first difference, printing the inputs.
//   usage: temporal_nr_surface_lane_rule_test          (no arguments; prints the number of combinations)
//
// Domain: srcY at offsets {0, 1, 2, 4, 8, 16, 24} from a page-aligned base, dstY at {0, 8, 16}, the chroma planes at {0, 4, 8, 16}; luma
// strides and pitches {0, 8, -16}, chroma strides and pitches {0, 8, 16}; interleaved {0, 1}.
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
    const std::vector<L> srcYOff = {0, 1, 2, 4, 8, 16, 24}, lumaOff = {0, 8, 16}, chromaOff = {0, 4, 8, 16}, lumaStep = {0, 8, -16},
                         chromaStep = {0, 8, 16};
    long long count = 0, ones[2] = {0, 0};
    for (int il = 0; il < 2; ++il)
    for (L sy : srcYOff)
    for (L dy : lumaOff) for (L su : chromaOff) for (L sv : chromaOff) for (L du : chromaOff) for (L dv : chromaOff)
    for (L ssY : lumaStep) for (L spY : lumaStep) for (L dsY : lumaStep) for (L dpY : lumaStep)
    for (L ssC : chromaStep) for (L spC : chromaStep) for (L dsC : chromaStep) for (L dpC : chromaStep) {
        if (il && (sv || dv)) continue;                              // an interleaved batch has no V plane
        const U srcY = kBase + (U)sy, dstY = kBase + (U)dy, srcU = kBase + (U)su, dstU = kBase + (U)du;
        const U srcV = il ? 0 : kBase + (U)sv, dstV = il ? 0 : kBase + (U)dv;
        const U cw = il ? 16 : 8;
        int want = rows_aligned(srcY, ssY, spY, 16) && rows_aligned(dstY, dsY, dpY, 16) && rows_aligned(srcU, ssC, spC, cw) && rows_aligned(dstU, dsC, dpC, cw);
        if (!il) want = want && rows_aligned(srcV, ssC, spC, cw) && rows_aligned(dstV, dsC, dpC, cw);
        const int is = temporal_nr_surface_vec16(RowsAt{srcY, 0, ssY, spY}, RowsAt{srcU, srcV, ssC, spC}, RowsAt{dstY, 0, dsY, dpY}, RowsAt{dstU, dstV, dsC, dpC}, il);
        ++count;
        ones[il] += is;
        if (want != is) {
            fprintf(stderr, "FAIL temporal nr surface vec: brute force %d, lane_rule.h gives %d for interleaved %d, inputs %lld %lld %lld %lld %lld %lld | %lld %lld %lld %lld | %lld %lld %lld %lld\n",
                    want, is, il, sy, dy, su, sv, du, dv, ssY, spY, dsY, dpY, ssC, spC, dsC, dpC);
            return 1;
        }
    }
    if (!ones[0] || !ones[1]) { fprintf(stderr, "FAIL temporal nr surface vec: the domain never selects the vector form\n"); return 1; }
    printf("temporal nr surface vec %lld combinations (%lld planar and %lld interleaved selections of the vector form), no difference\n", count, ones[0], ones[1]);
    return 0;
}
