// deband_plan.cpp -- the deband's offset tables (deband_plan.hpp).  Plain C++: no HIP.
#include "build_knobs.h"
#include "deband_plan.hpp"

#include <stdexcept>

namespace amt {

DebandTable deband_table(int plane, int W, int H, int R, uint32_t seed)
{
    if (plane < 0 || plane > 2) throw std::invalid_argument("deband_table: plane is 0 (Y), 1 (U) or 2 (V)");
    if (W < 1 || H < 1 || W > kDebandMaxSize || H > kDebandMaxSize) throw std::invalid_argument("deband_table: size outside 1..65534");
    if (R < 0 || R > kDebandMaxRadius) throw std::invalid_argument("deband_table: radius outside 0..31");
    DebandTable t;
    t.W = W; t.H = H; t.R = R;
    t.dx.resize((size_t)W * H);
    t.dy.resize((size_t)W * H);
    const uint32_t key = deband_mix(seed + 0x9e3779b9u * (uint32_t)(plane + 1));
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int lim = deband_lim(x, y, W, H, R);
            const uint32_t h = deband_mix(key ^ ((uint32_t)y << 16 | (uint32_t)x));
            const int a = (int)(h & 255), b = (int)((h >> 8) & 255);
            t.dx[(size_t)y * W + x] = (int8_t)(((a * (2 * lim + 1)) >> 8) - lim);
            t.dy[(size_t)y * W + x] = (int8_t)(((b * (2 * lim + 1)) >> 8) - lim);
        }
    return t;
}

long long deband_first_offset_outside(const int8_t* dx, const int8_t* dy, int W, int H, int R)
{
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int lim = deband_lim(x, y, W, H, R);
            const size_t i = (size_t)y * W + x;
            if (dx[i] > lim || dx[i] < -lim || dy[i] > lim || dy[i] < -lim) return (long long)i;
        }
    return -1;
}

std::vector<int8_t> deband_interleave(const std::vector<int8_t>& u, const std::vector<int8_t>& v, int W, int H, int pitch)
{
    if (W < 1 || H < 1 || pitch < 2 * W || u.size() != (size_t)W * H || v.size() != u.size())
        throw std::invalid_argument("deband_interleave: two tables of W x H entries and a pitch of at least 2 W");
    std::vector<int8_t> out((size_t)pitch * H, 0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            out[(size_t)y * pitch + 2 * x] = u[(size_t)y * W + x];
            out[(size_t)y * pitch + 2 * x + 1] = v[(size_t)y * W + x];
        }
    return out;
}

} // namespace amt
