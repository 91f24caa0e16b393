// deband_lane_rule_test.cpp -- deband_vec16 (amatsukaze_amd/csrc/lane_rule.h) against its definition, compiled with plain g++
// (tests/test_deband_host.py): 16-byte lanes exactly where 16 divides every base, frame stride and row pitch of the source's and the
// destination's luma and chroma planes.  One operand at a time is moved off a multiple of 64, the others stay on it.
#include <cstdio>

#include "lane_rule.h"

using namespace amt;

int main()
{
    long long checked = 0;
    const long long vals[] = {0, 16, 32, 8, 4, 2, 1, 48, 24, -16, -8, 1 << 20, (1ll << 33) + 16, (1ll << 33) + 8, (1ll << 33) + 1};
    for (int slot = 0; slot < 16; ++slot)
        for (long long v : vals) {
            long long o[16];
            for (int i = 0; i < 16; ++i) o[i] = 64;
            o[slot] = v;
            const RowsAt srcY{(uint64_t)o[0], (uint64_t)o[1], o[2], o[3]}, srcUV{(uint64_t)o[4], (uint64_t)o[5], o[6], o[7]};
            const RowsAt dstY{(uint64_t)o[8], (uint64_t)o[9], o[10], o[11]}, dstUV{(uint64_t)o[12], (uint64_t)o[13], o[14], o[15]};
            const int want = (unsigned long long)v % 16 == 0 ? 1 : 0;
            if (deband_vec16(srcY, srcUV, dstY, dstUV) != want) {
                printf("differs: operand %d = %lld, rule %d, definition %d\n", slot, v, deband_vec16(srcY, srcUV, dstY, dstUV), want);
                return 1;
            }
            ++checked;
        }
    printf("no difference in %lld selections\n", checked);
    return 0;
}
