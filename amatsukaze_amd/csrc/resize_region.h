// resize_region.h -- the LDS region of one wave of the resize's horizontal stage (resize_kernels.hip) and the rule that fits a wave's run
// of output columns into it.  Plain C++ with no include, so that it goes into kernels.hpp (the kernels size their LDS by it, the host
// refuses by it) and, through resize_plan.hpp, into tests/cpp/resize_plan_test.cpp under plain g++.  Defined in resize_plan.cpp.
#pragma once

namespace amt {

constexpr int kResizeRegionBytes = 2048;       // LDS of one wave of the horizontal stage: the source span of its run of output columns
constexpr int kResizeRegionSlack = 48;         // ... less the bytes in front of an aligned-down span (15) and behind it for zero taps (16 samples)

// The largest run of output columns (64 at the most) whose source span, start[last] + K - start[first], fits a wave's LDS region for
// every run of the row; 0: not even one column's window fits (the caller refuses)
int resize_columns_per_wave(const int* start, int D, int K, int es);

// The same for an interleaved UV row (resize_surface_kernels.hip), whose columns are PAIRS of 2 * es bytes and whose wave takes 32 of them
// at the most (64 lanes = 32 columns x 2 components): the span is 2 * es * (start[last] + K - start[first]) bytes.  Behind it a lane of the
// register forms reads KR - K zero taps, a pair each: 7 at the most (K = 1 in the form for K <= 8; the forms for 12 and 16 pad 3), 28
// bytes at es 2.  With the 15 bytes in front of an aligned-down span that is 43; the slack is the next multiple of 16.
constexpr int kResizeMaxZeroTaps = 7;
constexpr int kResizePairSlack = 48;
static_assert(15 + kResizeMaxZeroTaps * 2 * 2 <= kResizePairSlack && kResizePairSlack % 16 == 0, "every zero-tap read lands inside the region");
int resize_pair_columns_per_wave(const int* start, int D, int K, int es);

} // namespace amt
