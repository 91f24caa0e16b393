// edgelevel_lane_rule_test.cpp -- edgelevel_vec16 (amatsukaze_amd/csrc/lane_rule.h) against its definition, compiled with plain g++
// (tests/test_edgelevel_host.py): 16-byte lanes exactly where 16 divides every base, frame stride and row pitch of the source's and the
// destination's luma and chroma planes, the luma row is a whole number of pairs of containers and the chroma row a whole number of
// containers.  One operand at a time is moved off a multiple of 64, the others stay on it; both container sizes.
#include <cstdio>

#include "lane_rule.h"

using namespace amt;

int main()
{
    long long checked = 0;
    const long long vals[] = {0, 16, 32, 8, 4, 2, 1, 3, 6, 48, 24, -16, -8, 1 << 20, (1ll << 33) + 16, (1ll << 33) + 8, (1ll << 33) + 1};
    for (int es = 1; es <= 2; ++es)
        for (int slot = 0; slot < 18; ++slot)
            for (long long v : vals) {
                long long o[18];
                for (int i = 0; i < 18; ++i) o[i] = 64;
                o[slot] = v;
                const RowsAt srcY{(uint64_t)o[0], (uint64_t)o[1], o[2], o[3]}, srcUV{(uint64_t)o[4], (uint64_t)o[5], o[6], o[7]};
                const RowsAt dstY{(uint64_t)o[8], (uint64_t)o[9], o[10], o[11]}, dstUV{(uint64_t)o[12], (uint64_t)o[13], o[14], o[15]};
                // operands 16 and 17: the bytes of a luma and of a chroma row
                const unsigned long long u = (unsigned long long)v;
                const int want = slot < 16 ? (u % 16 == 0 ? 1 : 0) : slot == 16 ? (u % (2 * es) == 0 ? 1 : 0) : (u % es == 0 ? 1 : 0);
                const int got = edgelevel_vec16(es, srcY, srcUV, dstY, dstUV, o[16], o[17]);
                if (got != want) {
                    printf("differs: es %d, operand %d = %lld, rule %d, definition %d\n", es, slot, v, got, want);
                    return 1;
                }
                ++checked;
            }
    printf("no difference in %lld selections\n", checked);
    return 0;
}
