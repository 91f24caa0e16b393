// resize_surface_rules_test.cpp -- the two host rules of the resize on decoder surfaces, under plain g++ (with csrc/resize_plan.cpp):
//   resize_surface_rules_test                                  resize_surface_vec16 (csrc/lane_rule.h) against a brute-force check
//   resize_surface_rules_test pair S D kernel taps es ...       one line "S D kernel taps es K cpw" per group: K of the program and
//                                                              resize_pair_columns_per_wave of its windows (csrc/resize_region.h)
// Lane rule: the vector forms make 16-byte accesses at rows of the source, the intermediate and the destination, Y and UV (or U and V)
// alike, so the selection must be 1 exactly where every row start base + n * stride + y * pitch (n, y in 0..1) of every plane THERE IS
// is a multiple of 16 -- an interleaved surface has no V plane (base2 0), and a null plane counts as aligned.  Exits non-zero at the
// first difference, printing the inputs.
// Domain: luma planes at offsets {0, 2, 8, 16} from a page-aligned base, UV / U planes at {0, 8, 16}, V planes {none, 0, 8, 16}, the
// intermediate's at {0, 8}; strides and pitches {0, 8, 16, 48, -16} for the source's UV and the destination's luma.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lane_rule.h"
#include "resize_plan.hpp"

using namespace amt;
typedef uint64_t U;
typedef long long L;

static const U kBase = 0x7f3a00001000ull;

static bool rows_aligned(U base, L stride, L pitch)
{
    if (!base) return true;                         // no such plane
    for (int n = 0; n < 2; ++n)
        for (int y = 0; y < 2; ++y)
            if ((base + (U)(n * stride) + (U)(y * pitch)) % 16) return false;
    return true;
}

static int lane_rule()
{
    const std::vector<L> lumaOff = {0, 2, 8, 16}, uvOff = {0, 8, 16}, vOff = {-1, 0, 8, 16}, midOff = {0, 8}, step = {0, 8, 16, 48, -16};
    long long count = 0, ones = 0;
    for (L sy : lumaOff) for (L dy : lumaOff) for (L su : uvOff) for (L du : uvOff) for (L sv : vOff) for (L dv : vOff)
    for (L my : midOff) for (L mc : midOff)
    for (L ssC : step) for (L spC : step) for (L dsY : step) for (L dpY : step) {
        const U sV = sv < 0 ? 0 : kBase + (U)sv, dV = dv < 0 ? 0 : kBase + (U)dv, mV = sv < 0 ? 0 : kBase + (U)mc + 64;
        const RowsAt srcY{kBase + (U)sy, 0, 64, 32}, srcUV{kBase + (U)su, sV, ssC, spC}, midY{kBase + (U)my, 0, 32, 16}, midUV{kBase + (U)mc, mV, 32, 16},
                     dstY{kBase + (U)dy, 0, dsY, dpY}, dstUV{kBase + (U)du, dV, 32, 16};
        const int want = rows_aligned(srcY.base, 64, 32) && rows_aligned(srcUV.base, ssC, spC) && rows_aligned(srcUV.base2, ssC, spC) &&
                         rows_aligned(midY.base, 32, 16) && rows_aligned(midUV.base, 32, 16) && rows_aligned(midUV.base2, 32, 16) &&
                         rows_aligned(dstY.base, dsY, dpY) && rows_aligned(dstUV.base, 32, 16) && rows_aligned(dstUV.base2, 32, 16);
        const int is = resize_surface_vec16(srcY, srcUV, midY, midUV, dstY, dstUV);
        ++count;
        ones += is;
        if (want != is) {
            fprintf(stderr, "FAIL resize surface vec: brute force %d, lane_rule.h gives %d for inputs %lld %lld %lld %lld %lld %lld | %lld %lld | %lld %lld %lld %lld\n",
                    want, is, sy, dy, su, du, sv, dv, my, mc, ssC, spC, dsY, dpY);
            return 1;
        }
    }
    if (!ones || ones == count) { fprintf(stderr, "FAIL resize surface vec: the domain holds only one answer\n"); return 1; }
    printf("resize surface vec %lld combinations (%lld vector), no difference\n", count, ones);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 1) return lane_rule();
    if (strcmp(argv[1], "pair") || (argc - 2) % 5) { fprintf(stderr, "usage: resize_surface_rules_test [pair S D kernel taps es ...]\n"); return 2; }
    for (int i = 2; i < argc; i += 5) {
        const int S = atoi(argv[i]), D = atoi(argv[i + 1]), kernel = atoi(argv[i + 2]), taps = atoi(argv[i + 3]), es = atoi(argv[i + 4]);
        const ResizeProgram p = resize_program(S, D, kernel, taps);
        printf("%d %d %d %d %d %d %d\n", S, D, kernel, taps, es, p.K, resize_pair_columns_per_wave(p.start.data(), D, p.K, es));
    }
    return 0;
}
