// deband_plan.hpp -- the host plan of the deband ("parity unpinned"): the offset table of one plane, static over
// frames and a function of the plane's size, its radius, the plane's number and the seed alone.  For the pixel (x, y) of plane p
// (0 Y, 1 U, 2 V) of W x H containers with radius R (the caller's for luma, half of it for chroma):
//   lim = min(R, x, W - 1 - x, y, H - 1 - y);  key = mix(seed + 0x9e3779b9 * (p + 1));  h = mix(key ^ (y << 16 | x));
//   dx = (((h & 255) * (2 lim + 1)) >> 8) - lim,  dy = ((((h >> 8) & 255) * (2 lim + 1)) >> 8) - lim,
// everything uint32 with wrap-around, mix being the 32-bit finaliser below.  |dx|, |dy| <= lim, so the four references
// (x + dx, y + dy), (x - dx, y - dy), (x - dy, y + dx), (x + dy, y - dx) lie inside the plane.  No HIP in this file or in
// deband_plan.cpp: tests/cpp/deband_plan_test.cpp compiles the pair with plain g++.
#pragma once

#include <cstdint>
#include <vector>

namespace amt {

constexpr int kDebandMaxRadius = 31;
constexpr int kDebandMaxSize = 65534;            // the hash key packs y << 16 | x

inline uint32_t deband_mix(uint32_t v)
{
    v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;
    return v;
}
inline int deband_lim(int x, int y, int W, int H, int R)
{
    int l = R;
    if (x < l) l = x;
    if (W - 1 - x < l) l = W - 1 - x;
    if (y < l) l = y;
    if (H - 1 - y < l) l = H - 1 - y;
    return l;
}
// the radius of plane p for the caller's figure
inline int deband_plane_radius(int plane, int radius) { return plane ? radius >> 1 : radius; }

struct DebandTable {
    int W = 0, H = 0, R = 0;
    std::vector<int8_t> dx, dy;                  // [H][W], row-major
};
// The table of plane `plane` (0..2), W x H containers, R = the PLANE's radius (0..31).  Throws std::invalid_argument for a plane outside
// 0..2, a size outside 1..65534 or a radius outside 0..31
DebandTable deband_table(int plane, int W, int H, int R, uint32_t seed);
// The first entry (row-major index) of a caller's table whose |dx| or |dy| exceeds lim(x, y), or -1 where every entry is inside
long long deband_first_offset_outside(const int8_t* dx, const int8_t* dy, int W, int H, int R);
// One of dx / dy of the interleaved UV plane of a decoder surface, which the surface kernels walk as one plane of 2 W containers by H
// rows: u's entry at 2x and v's at 2x + 1 of rows `pitch` entries apart (pitch >= 2 W; the entries behind 2 W are zero).  u and v are
// W x H, row-major.  Throws std::invalid_argument otherwise
std::vector<int8_t> deband_interleave(const std::vector<int8_t>& u, const std::vector<int8_t>& v, int W, int H, int pitch);

} // namespace amt
