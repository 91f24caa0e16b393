// deband_interleave_test.cpp -- the interleaved UV table of the deband on decoder surfaces (deband_interleave, amatsukaze_amd/csrc/
// deband_plan.cpp) as a stand-alone program, compiled with plain g++ (tests/test_deband_surfaces_host.py; no HIP, no Python inside).
//   usage: deband_interleave_test                        self-checks: the padding, the refusals, and that every reference of the UV plane
//                                                        walked as one plane stays inside its row and on its own component; prints
//                                                        "deband interleave ok"
//          deband_interleave_test W H R seed pitch       W x H and R are a CHROMA plane's: pitch * H bytes of the interleaved dx, then of
//                                                        dy, raw int8, to stdout
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "deband_plan.hpp"

using namespace amt;

static int fail(const char* what, int W, int H, int R)
{
    fprintf(stderr, "FAIL %s at %d x %d, radius %d\n", what, W, H, R);
    return 1;
}

static int self_checks()
{
    static const int sizes[][2] = {{1, 1}, {4, 3}, {65, 49}, {145, 99}};
    for (const auto& wh : sizes)
        for (int R : {0, 12, 15}) {
            const int W = wh[0], H = wh[1], pitch = (2 * W + 15) & ~15;
            const DebandTable u = deband_table(1, W, H, R, 3), v = deband_table(2, W, H, R, 3);
            const std::vector<int8_t> dx = deband_interleave(u.dx, v.dx, W, H, pitch), dy = deband_interleave(u.dy, v.dy, W, H, pitch);
            if (dx.size() != (size_t)pitch * H || dy.size() != dx.size()) return fail("size", W, H, R);
            for (int y = 0; y < H; ++y)
                for (int c = 0; c < pitch; ++c) {
                    const int ex = dx[(size_t)y * pitch + c], ey = dy[(size_t)y * pitch + c];
                    if (c >= 2 * W) {
                        if (ex || ey) return fail("padding is not zero", W, H, R);
                        continue;
                    }
                    const DebandTable& t = c & 1 ? v : u;
                    if (ex != t.dx[(size_t)y * W + c / 2] || ey != t.dy[(size_t)y * W + c / 2]) return fail("entry", W, H, R);
                    // the cell's references in containers of the UV row: 2 containers to a unit of a horizontal offset
                    const int xs[4] = {c + 2 * ex, c - 2 * ex, c - 2 * ey, c + 2 * ey}, ys[4] = {y + ey, y - ey, y + ex, y - ex};
                    for (int k = 0; k < 4; ++k) {
                        if (xs[k] < 0 || xs[k] >= 2 * W || ys[k] < 0 || ys[k] >= H) return fail("reference outside the UV plane", W, H, R);
                        if ((xs[k] & 1) != (c & 1)) return fail("reference on the other component", W, H, R);
                        if (abs(xs[k] - c) > 2 * R || abs(ys[k] - y) > R) return fail("reference outside the staged halo", W, H, R);
                    }
                }
        }
    const std::vector<int8_t> a(12, 0), b(11, 0);
    for (int k = 0; k < 4; ++k) {
        bool refused = false;
        try {
            if (k == 0) deband_interleave(a, b, 4, 3, 16);                  // tables of different sizes
            if (k == 1) deband_interleave(a, a, 4, 3, 7);                   // a pitch below 2 W
            if (k == 2) deband_interleave(a, a, 3, 3, 16);                  // not W x H entries
            if (k == 3) deband_interleave(a, a, 0, 3, 16);
        } catch (const std::invalid_argument&) { refused = true; }
        if (!refused) return fail("a bad argument was taken", k, 0, 0);
    }
    puts("deband interleave ok");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 1) return self_checks();
    if (argc != 6) return 2;
    const int W = atoi(argv[1]), H = atoi(argv[2]), R = atoi(argv[3]), pitch = atoi(argv[5]);
    const uint32_t seed = (uint32_t)strtoul(argv[4], nullptr, 0);
    const DebandTable u = deband_table(1, W, H, R, seed), v = deband_table(2, W, H, R, seed);
    for (int k = 0; k < 2; ++k) {
        const std::vector<int8_t> t = deband_interleave(k ? u.dy : u.dx, k ? v.dy : v.dx, W, H, pitch);
        if (fwrite(t.data(), 1, t.size(), stdout) != t.size()) return 3;
    }
    return 0;
}
