// deband_plan_test.cpp -- the deband's host plan (amatsukaze_amd/csrc/deband_plan.cpp) as a stand-alone program, compiled with plain g++
// (tests/test_deband_host.py; no HIP, no Python inside).
//   usage: deband_plan_test                              self-checks: every offset inside lim, lim itself, the check of a caller's table,
//                                                        the refusals; prints "deband plan ok"
//          deband_plan_test plane W H R seed [...]       per quintuple the table's W * H bytes of dx, then of dy, raw int8, to stdout
//                                                        (W x H and R are the PLANE's size and radius)
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    static const int sizes[][2] = {{1, 1}, {2, 2}, {8, 6}, {65, 17}, {130, 34}, {640, 360}};
    long long tables = 0;
    for (const auto& wh : sizes)
        for (int R : {0, 1, 12, 25, 31})
            for (int plane = 0; plane < 3; ++plane) {
                const int W = wh[0], H = wh[1];
                const DebandTable t = deband_table(plane, W, H, R, 7u * (unsigned)plane);
                if (t.W != W || t.H != H || t.R != R || t.dx.size() != (size_t)W * H || t.dy.size() != (size_t)W * H) return fail("shape", W, H, R);
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) {
                        const int lim = deband_lim(x, y, W, H, R), dx = t.dx[(size_t)y * W + x], dy = t.dy[(size_t)y * W + x];
                        if (lim < 0 || lim > R || lim > x || lim > y || lim > W - 1 - x || lim > H - 1 - y) return fail("lim", W, H, R);
                        if (abs(dx) > lim || abs(dy) > lim) return fail("offset outside lim", W, H, R);
                        // all four references inside the plane
                        const int xs[4] = {x + dx, x - dx, x - dy, x + dy}, ys[4] = {y + dy, y - dy, y + dx, y - dx};
                        for (int k = 0; k < 4; ++k)
                            if (xs[k] < 0 || xs[k] >= W || ys[k] < 0 || ys[k] >= H) return fail("reference outside the plane", W, H, R);
                    }
                if (deband_first_offset_outside(t.dx.data(), t.dy.data(), W, H, R) != -1) return fail("own table refused", W, H, R);
                ++tables;
            }
    // a caller's table: one entry beyond lim is found, at its place; entries at +-lim pass
    {
        const int W = 12, H = 10, R = 3;
        DebandTable t = deband_table(0, W, H, R, 1);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const int lim = deband_lim(x, y, W, H, R);
                t.dx[(size_t)y * W + x] = (int8_t)((x + y) & 1 ? lim : -lim);
                t.dy[(size_t)y * W + x] = (int8_t)((x + y) & 1 ? -lim : lim);
            }
        if (deband_first_offset_outside(t.dx.data(), t.dy.data(), W, H, R) != -1) return fail("offsets at the limit refused", W, H, R);
        const size_t spots[] = {0, (size_t)W - 1, (size_t)5 * W + 6, (size_t)W * H - 1};
        for (size_t at : spots)
            for (int which = 0; which < 4; ++which) {
                DebandTable u = t;
                const int lim = deband_lim((int)(at % W), (int)(at / W), W, H, R);
                (which & 1 ? u.dy : u.dx)[at] = (int8_t)(which & 2 ? -(lim + 1) : lim + 1);
                if (deband_first_offset_outside(u.dx.data(), u.dy.data(), W, H, R) != (long long)at) return fail("offset beyond lim accepted", W, H, R);
            }
    }
    if (deband_plane_radius(0, 25) != 25 || deband_plane_radius(1, 25) != 12 || deband_plane_radius(2, 1) != 0) return fail("plane radius", 0, 0, 25);
    if (deband_mix(0) != 0 || deband_mix(1) == 1) return fail("mix", 0, 0, 0);
    try { deband_table(3, 8, 8, 1, 0); return fail("plane 3 accepted", 8, 8, 1); } catch (const std::invalid_argument&) {}
    try { deband_table(0, 0, 8, 1, 0); return fail("empty plane accepted", 0, 8, 1); } catch (const std::invalid_argument&) {}
    try { deband_table(0, 65535, 8, 1, 0); return fail("width 65535 accepted", 65535, 8, 1); } catch (const std::invalid_argument&) {}
    try { deband_table(0, 8, 8, 32, 0); return fail("radius 32 accepted", 8, 8, 32); } catch (const std::invalid_argument&) {}
    try { deband_table(0, 8, 8, -1, 0); return fail("radius -1 accepted", 8, 8, -1); } catch (const std::invalid_argument&) {}
    printf("deband plan ok: %lld tables\n", tables);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 1) return self_checks();
    if ((argc - 1) % 5) { fprintf(stderr, "usage: deband_plan_test [plane W H R seed]...\n"); return 2; }
    for (int a = 1; a + 4 < argc; a += 5) {
        const DebandTable t = deband_table(atoi(argv[a]), atoi(argv[a + 1]), atoi(argv[a + 2]), atoi(argv[a + 3]), (uint32_t)strtoul(argv[a + 4], nullptr, 10));
        if (fwrite(t.dx.data(), 1, t.dx.size(), stdout) != t.dx.size() || fwrite(t.dy.data(), 1, t.dy.size(), stdout) != t.dy.size()) return 3;
    }
    return 0;
}
