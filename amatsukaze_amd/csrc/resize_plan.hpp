// resize_plan.hpp -- the host plan of the resize ("parity unpinned"): the program of one axis, S source samples to
// D destination samples with a Blackman, Lanczos or bilinear kernel, as integers.  Output sample i is
//   clamp((sum_j coeff[i * K + j] * s[start[i] + j] + 8192) >> 14, 0, maxv),
// every row of coeff sums to 16384 and every window [start[i], start[i] + K) lies inside the axis.  Everything is computed in double and
// quantised once; the kernels see integers only.  No HIP in this file or in resize_plan.cpp: tests/cpp/resize_plan_test.cpp compiles the
// pair with plain g++.
#pragma once

#include <vector>

#include "resize_region.h"      // resize_columns_per_wave: which run of output columns a wave of the horizontal stage takes

namespace amt {

enum ResizeKernel { kResizeBlackman = 0, kResizeLanczos = 1, kResizeBilinear = 2 };   // AMTGPU_RESIZE_*

constexpr int kResizeOne = 16384, kResizeShift = 14;

struct ResizeProgram {
    int S = 0, D = 0, K = 0;
    std::vector<int> start;      // [D]
    std::vector<int> coeff;      // [D][K]: coeff[i * K + j] belongs to source position start[i] + j
};

// the kernel's default taps (blackman 4, lanczos 3, bilinear 1); 0 for an unknown kernel
int resize_default_taps(int kernel);
// k(x) of the rule, in double
double resize_kernel_value(int kernel, int taps, double x);
// The program of one axis.  taps <= 0: the kernel's default (bilinear has taps 1 whatever is passed).  Throws std::invalid_argument for
// sizes below 1, an unknown kernel or taps above 64
ResizeProgram resize_program(int S, int D, int kernel, int taps);
// Over the program's rows: the largest sum of positive coefficients and the smallest sum of negative ones
struct ResizeSums { long long positive, negative; };
ResizeSums resize_program_sums(const ResizeProgram& p);
// May the int32 accumulator of the sample rule hold every sum at samples of 0 .. (1 << bits) - 1: positive * maxv + 8192 <= INT32_MAX and
// negative * maxv + 8192 >= INT32_MIN
bool resize_program_fits_int32(const ResizeProgram& p, int bits);

} // namespace amt
