// resize_plan.cpp -- the resize's host plan (resize_plan.hpp).  Plain C++, no HIP.
#include "build_knobs.h"
#include "resize_plan.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <stdexcept>
#include <string>

namespace amt {

namespace {
const double kPi = 3.14159265358979323846;
}

int resize_default_taps(int kernel)
{
    return kernel == kResizeBlackman ? 4 : kernel == kResizeLanczos ? 3 : kernel == kResizeBilinear ? 1 : 0;
}

double resize_kernel_value(int kernel, int taps, double x)
{
    const double ax = std::fabs(x);
    if (ax >= (double)taps) return 0.0;
    if (ax == 0.0) return 1.0;
    if (kernel == kResizeBilinear) return std::max(0.0, 1.0 - ax);
    const double px = kPi * ax;
    if (kernel == kResizeBlackman) return std::sin(px) / px * (0.42 + 0.5 * std::cos(px / taps) + 0.08 * std::cos(2 * px / taps));
    return std::sin(px) / px * std::sin(px / taps) / (px / taps);
}

ResizeProgram resize_program(int S, int D, int kernel, int taps)
{
    if (S < 1 || D < 1) throw std::invalid_argument("resize: sizes must be positive");
    if (!resize_default_taps(kernel)) throw std::invalid_argument("resize: unknown kernel");
    if (taps <= 0 || kernel == kResizeBilinear) taps = resize_default_taps(kernel);
    if (taps > 64) throw std::invalid_argument("resize: taps must be at most 64");
    const double scale = (double)D / (double)S, fstep = scale < 1.0 ? scale : 1.0, support = (double)taps / fstep;
    const long long K0 = (long long)std::ceil(2 * support);
    const int K = (int)std::min<long long>(K0, S);
    ResizeProgram prog;
    prog.S = S; prog.D = D; prog.K = K;
    prog.start.assign((size_t)D, 0);
    prog.coeff.assign((size_t)D * K, 0);
    std::vector<double> folded((size_t)K);
    std::vector<int> C((size_t)K);
    for (int i = 0; i < D; ++i) {
        const double c = ((double)i + 0.5) / scale - 0.5;
        const long long lo = (long long)std::floor(c - support) + 1;
        auto clampS = [&](long long p) { return (int)std::min<long long>(std::max<long long>(p, 0), S - 1); };
        const int first = clampS(lo), last = clampS(lo + K0 - 1), n = last - first + 1;       // the positions that take weight: n <= K
        std::fill(folded.begin(), folded.end(), 0.0);
        double total = 0.0;
        for (long long p = lo; p < lo + K0; ++p) {
            const double w = resize_kernel_value(kernel, taps, ((double)p - c) * fstep);
            total += w;
            folded[(size_t)(clampS(p) - first)] += w;
        }
        int sum = 0, best = 0;
        for (int j = 0; j < n; ++j) {
            C[(size_t)j] = (int)std::floor(folded[(size_t)j] / total * (double)kResizeOne + 0.5);
            sum += C[(size_t)j];
            if (C[(size_t)j] > C[(size_t)best]) best = j;
        }
        C[(size_t)best] += kResizeOne - sum;
        const int start = (int)std::min<long long>(std::max<long long>(lo, 0), S - K);
        prog.start[(size_t)i] = start;
        for (int j = 0; j < n; ++j) {
            const int at = first + j - start;
            if (at < 0 || at >= K) {
                if (C[(size_t)j]) throw std::logic_error("resize: a coefficient outside its window at output sample " + std::to_string(i));
                continue;
            }
            prog.coeff[(size_t)i * K + at] = C[(size_t)j];
        }
    }
    return prog;
}

ResizeSums resize_program_sums(const ResizeProgram& p)
{
    ResizeSums s{0, 0};
    for (int i = 0; i < p.D; ++i) {
        long long pos = 0, neg = 0;
        for (int j = 0; j < p.K; ++j) {
            const int c = p.coeff[(size_t)i * p.K + j];
            (c > 0 ? pos : neg) += c;
        }
        s.positive = std::max(s.positive, pos);
        s.negative = std::min(s.negative, neg);
    }
    return s;
}

bool resize_program_fits_int32(const ResizeProgram& p, int bits)
{
    const long long maxv = (1LL << bits) - 1, half = kResizeOne / 2;
    const ResizeSums s = resize_program_sums(p);
    // (sums of up to K coefficients of any int: the products are formed in 128 bits' worth of care -- a forged program may hold INT_MAX)
    const long double hi = (long double)s.positive * (long double)maxv + (long double)half, lo = (long double)s.negative * (long double)maxv + (long double)half;
    return hi <= (long double)INT_MAX && lo >= (long double)INT_MIN;
}

int resize_columns_per_wave(const int* start, int D, int K, int es)
{
    for (int cpw = 64; cpw >= 1; cpw >>= 1) {
        bool fits = true;
        for (int c0 = 0; c0 < D && fits; c0 += cpw) {
            const int last = (c0 + cpw < D ? c0 + cpw : D) - 1;
            fits = (long long)(start[last] + K - start[c0]) * es + kResizeRegionSlack <= kResizeRegionBytes;
        }
        if (fits) return cpw;
    }
    return 0;
}

int resize_pair_columns_per_wave(const int* start, int D, int K, int es)
{
    for (int cpw = 32; cpw >= 1; cpw >>= 1) {
        bool fits = true;
        for (int c0 = 0; c0 < D && fits; c0 += cpw) {
            const int last = (c0 + cpw < D ? c0 + cpw : D) - 1;
            fits = (long long)(start[last] + K - start[c0]) * 2 * es + kResizePairSlack <= kResizeRegionBytes;
        }
        if (fits) return cpw;
    }
    return 0;
}

} // namespace amt
