// resize_plan_test.cpp -- the resize's host plan (amatsukaze_amd/csrc/resize_plan.cpp) as a stand-alone program, compiled with plain g++
// (tests/test_resize_host.py; no HIP, no Python inside).
//   usage: resize_plan_test                          self-checks: every row sums to 16384, every window inside the axis, the int32 check at
//                                                    16 bits, and its refusal of programs made to exceed it; prints "resize plan ok"
//          resize_plan_test S D kernel taps [...]    one line per quadruple: "S D kernel taps K | start[0..D) | coeff[0..D*K)"
//                                                    (kernel 0 blackman, 1 lanczos, 2 bilinear; taps 0: the kernel's default)
//          resize_plan_test cpw S D kernel taps es [...]   one line per quintuple: "S D kernel taps es K cpw", cpw being
//                                                    resize_columns_per_wave of the program at containers of es bytes (0: refused)
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "resize_plan.hpp"

using namespace amt;

static int fail(const char* what, int S, int D, int kernel)
{
    fprintf(stderr, "FAIL %s at %d -> %d, kernel %d\n", what, S, D, kernel);
    return 1;
}

static int self_checks()
{
    static const int pairs[][2] = {{1920, 1280}, {1080, 720}, {1440, 1280}, {272, 182}, {136, 91}, {32, 50}, {16, 8}, {8, 4}, {4, 2}, {64, 64}, {48, 32}, {2, 2}, {1, 7}, {4096, 2}};
    long long programs = 0;
    for (const auto& sd : pairs)
        for (int kernel = 0; kernel < 3; ++kernel) {
            const ResizeProgram p = resize_program(sd[0], sd[1], kernel, 0);
            if (p.K < 1 || p.K > p.S || (int)p.start.size() != p.D || (int)p.coeff.size() != p.D * p.K) return fail("shape", sd[0], sd[1], kernel);
            for (int i = 0; i < p.D; ++i) {
                long long sum = 0;
                for (int j = 0; j < p.K; ++j) sum += p.coeff[(size_t)i * p.K + j];
                if (sum != kResizeOne) return fail("row sum", sd[0], sd[1], kernel);
                if (p.start[(size_t)i] < 0 || p.start[(size_t)i] + p.K > p.S) return fail("window", sd[0], sd[1], kernel);
            }
            for (int bits = 8; bits <= 16; ++bits)
                if (!resize_program_fits_int32(p, bits)) return fail("int32 check", sd[0], sd[1], kernel);
            ++programs;
        }
    // programs made to exceed the accumulator: rows still sum to 16384
    ResizeProgram big;
    big.S = 2; big.D = 1; big.K = 2; big.start = {0};
    big.coeff = {kResizeOne + 40000, -40000};                           // 56 384 * 65 535 + 8192 > INT32_MAX
    if (resize_program_fits_int32(big, 16)) return fail("forged positive sum accepted", 2, 1, -1);
    if (!resize_program_fits_int32(big, 14)) return fail("forged positive sum refused at 14 bits, where it fits", 2, 1, -1);
    big.coeff = {-40000, kResizeOne + 40000};
    if (resize_program_fits_int32(big, 16)) return fail("forged positive sum accepted", 2, 1, -1);
    big.S = 3; big.K = 3;
    big.coeff = {-33000, 2 * kResizeOne, -kResizeOne + 33000};
    {
        const ResizeSums s = resize_program_sums(big);
        if (s.positive != 2 * kResizeOne + (33000 - kResizeOne) || s.negative != -33000) return fail("sums of a forged program", 3, 1, -1);
    }
    big.coeff = {-33000, kResizeOne + 33000, 0};                        // -33 000 * 65 535 + 8192 < INT32_MIN
    if (resize_program_fits_int32(big, 16)) return fail("forged negative sum accepted", 3, 1, -1);
    big.coeff = {INT_MAX, INT_MIN + kResizeOne + 1, 0};
    if (resize_program_fits_int32(big, 8)) return fail("forged extreme program accepted", 3, 1, -1);
    for (int kernel : {-1, 3})
        try { resize_program(8, 8, kernel, 0); return fail("unknown kernel accepted", 8, 8, kernel); } catch (const std::invalid_argument&) {}
    try { resize_program(0, 8, 0, 0); return fail("empty axis accepted", 0, 8, 0); } catch (const std::invalid_argument&) {}
    try { resize_program(8, 8, 0, 65); return fail("65 taps accepted", 8, 8, 0); } catch (const std::invalid_argument&) {}
    printf("resize plan ok: %lld programs\n", programs);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 1) return self_checks();
    if (!strcmp(argv[1], "cpw")) {
        if ((argc - 2) % 5) { fprintf(stderr, "usage: resize_plan_test cpw [S D kernel taps es]...\n"); return 2; }
        for (int a = 2; a + 4 < argc; a += 5) {
            const int S = atoi(argv[a]), D = atoi(argv[a + 1]), kernel = atoi(argv[a + 2]), taps = atoi(argv[a + 3]), es = atoi(argv[a + 4]);
            const ResizeProgram p = resize_program(S, D, kernel, taps);
            printf("%d %d %d %d %d %d %d\n", S, D, kernel, taps, es, p.K, resize_columns_per_wave(p.start.data(), p.D, p.K, es));
        }
        return 0;
    }
    if ((argc - 1) % 4) { fprintf(stderr, "usage: resize_plan_test [S D kernel taps]...\n"); return 2; }
    for (int a = 1; a + 3 < argc; a += 4) {
        const int S = atoi(argv[a]), D = atoi(argv[a + 1]), kernel = atoi(argv[a + 2]), taps = atoi(argv[a + 3]);
        const ResizeProgram p = resize_program(S, D, kernel, taps);
        printf("%d %d %d %d %d |", S, D, kernel, taps, p.K);
        for (int v : p.start) printf(" %d", v);
        printf(" |");
        for (int v : p.coeff) printf(" %d", v);
        printf("\n");
    }
    return 0;
}
