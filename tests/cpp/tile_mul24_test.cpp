// The operand limits of the tile kernels' 24-bit multiplies (amatsukaze_amd/csrc/eval_tiles.hpp: mul24, tile_mul24_operands_ok,
// tile_slots_ok), on the host.
//
// On the device mul24(a, b) is v_mul_u32_u24: the low 32 bits of (a & 0xFFFFFF) * (b & 0xFFFFFF).  That is a * b exactly when both
// operands are below 2^24 -- whatever the size of the product -- and something else as soon as one is not.  This program
//   1. checks the guard at its limits: pitch 2^24 - 1 / 2^24 / 2^24 + 1 bytes, row numbers 2^24 - 1 / 2^24, row_step, logo
//      dimensions, slot counts 2^20 - 1 / 2^20;
//   2. replays the instruction's arithmetic (mul24_device below) against plain multiplication and against the header's host form over
//      the operands the guard admits: every staging unit of every tile shape (tile_unit), and row offsets (row0 + y * step) * pitch
//      with pitches and rows up to the limits -- products far beyond 2^24, compared modulo 2^32 as the kernels use them;
//   3. shows that the limit is the right one: at an operand of 2^24 the instruction's result differs from the product.
// Exits non-zero at the first difference.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "eval_tiles.hpp"

using namespace amt;

static uint32_t mul24_device(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)(a & 0xFFFFFFu) * (uint64_t)(b & 0xFFFFFFu)); }

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

// tile_unit() with the device's multiply
static TileUnit tile_unit_device(const TileDesc& T, int u, int w)
{
    const int last = T.nrows * T.ncol4 - 1;
    u = u < last ? u : (last < 0 ? 0 : last);
    const int row = (int)(mul24_device((uint32_t)u, (uint32_t)T.rcp) >> 16);
    const int c4 = u - (int)mul24_device((uint32_t)row, (uint32_t)T.ncol4);
    const int x = T.x0 + 4 * c4;
    const int xs = x < w - 4 ? x : w - 4;
    return TileUnit{T.y0 + row, xs, (int)mul24_device((uint32_t)row, (uint32_t)T.tp) + (xs - T.x0)};
}

int main()
{
    const long long M = 1LL << 24;
    // ---- 1. the guard at its limits ----
    CHECK(kMul24Limit == M && kTileSlotLimit == (1LL << 20));
    CHECK(tile_mul24_operands_ok(M - 1, 1, 1000, 256, 128));
    CHECK(!tile_mul24_operands_ok(M, 1, 1000, 256, 128));
    CHECK(!tile_mul24_operands_ok(M + 1, 1, 1000, 256, 128));
    CHECK(!tile_mul24_operands_ok(0, 1, 1000, 256, 128) && !tile_mul24_operands_ok(-8, 1, 1000, 256, 128));
    CHECK(tile_mul24_operands_ok(1472, 1, M - 1, 256, 128));
    CHECK(!tile_mul24_operands_ok(1472, 1, M, 256, 128) && !tile_mul24_operands_ok(1472, 1, M + 1, 256, 128));
    CHECK(!tile_mul24_operands_ok(1472, 1, -1, 256, 128));
    CHECK(tile_mul24_operands_ok(1472, 2, 1000, 256, 128) && !tile_mul24_operands_ok(1472, 0, 1000, 256, 128) && !tile_mul24_operands_ok(1472, M, 1000, 256, 128));
    CHECK(tile_mul24_operands_ok(1472, 1, 1000, 65536, 65536) && !tile_mul24_operands_ok(1472, 1, 1000, 65537, 128) && !tile_mul24_operands_ok(1472, 1, 1000, 256, 65537));
    CHECK(!tile_mul24_operands_ok(1472, 1, 1000, 0, 128) && !tile_mul24_operands_ok(1472, 1, 1000, 256, 0));
    CHECK(tile_slots_ok((1 << 20) - 1) && !tile_slots_ok(1 << 20) && !tile_slots_ok((1 << 20) + 1) && tile_slots_ok(0) && !tile_slots_ok(-1));
    CHECK(tile_slots_ok(64) && !tile_slots_ok(1LL << 31));

    // ---- 2a. every staging unit of every tile shape: device arithmetic == host form == division ----
    long long units = 0;
    for (int ncol4 = 1; ncol4 <= kTileLanes * kTileUnits; ++ncol4)
        for (int nrows = 1; nrows * ncol4 <= kTileLanes * kTileUnits && nrows * ncol4 * 4 <= kTileCap; ++nrows)
            for (int tp = ncol4 * 4; tp * nrows <= kTileCap && tp < ncol4 * 4 + 32; tp += 2) {
                TileDesc T{6, 3, nrows, ncol4, tp, 64, (65536 + ncol4 - 1) / ncol4, 0};
                for (int w : {T.x0 + 4 * ncol4, T.x0 + 4 * ncol4 - 2, 65536})
                    for (int u = 0; u < kTileLanes * kTileUnits; ++u) {
                        const TileUnit a = tile_unit(T, u, w), d = tile_unit_device(T, u, w);
                        const int uc = u < nrows * ncol4 - 1 ? u : nrows * ncol4 - 1, row = uc / ncol4;
                        ++units;
                        if (a.y != d.y || a.xs != d.xs || a.lds != d.lds || a.y != T.y0 + row) {
                            std::printf("tile_unit differs: ncol4 %d nrows %d tp %d w %d u %d\n", ncol4, nrows, tp, w, u);
                            return 1;
                        }
                    }
            }
    // ---- 2b. row offsets and coefficient offsets over the admitted operands (products up to 2^48, used modulo 2^32) ----
    const uint32_t edge[] = {0u, 1u, 2u, 3u, 255u, 256u, 1079u, 1472u, 2100u, 2303u, 4095u, 8192u, 65535u, 65536u, 65537u, (1u << 20) - 1, 1u << 20,
                             (1u << 23) - 1, 1u << 23, (1u << 23) + 1, (1u << 24) - 2, (1u << 24) - 1};
    long long prods = 0;
    for (uint32_t a : edge)
        for (uint32_t b : edge) {
            ++prods;
            if (mul24_device(a, b) != a * b || mul24(a, b) != a * b) { std::printf("mul24 differs at %u x %u\n", a, b); return 1; }
        }
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    for (int i = 0; i < 2000000; ++i) {
        const uint32_t pitch = (uint32_t)(next() % (M - 1)) + 1, step = 1 + (uint32_t)(next() & 1), y = (uint32_t)(next() % 65536), w = (uint32_t)(next() % 65536) + 1;
        const uint32_t row0 = (uint32_t)(next() % (M - (long long)y * step));          // row0 + y * step < 2^24: what last_row < 2^24 admits
        const uint32_t rowd = row0 + mul24_device(y, step), row = row0 + y * step;
        ++prods;
        if (rowd != row || mul24_device(rowd, pitch) != row * pitch || mul24(row, pitch) != row * pitch || mul24_device(y, w) != y * w) {
            std::printf("row offset differs: pitch %u step %u y %u row0 %u w %u\n", pitch, step, y, row0, w);
            return 1;
        }
    }
    // the issue's frame: pitch 8192 bytes, rows from 2100 on -- offsets beyond 2^24, exact
    CHECK(mul24_device(2100u, 8192u) == 2100u * 8192u && 2100u * 8192u > (1u << 24));
    // ---- 3. one operand at the limit: the instruction no longer multiplies ----
    CHECK(mul24_device(1u << 24, 3u) != (1u << 24) * 3u);
    CHECK(mul24_device((1u << 24) + 1, 3u) == 3u);
    CHECK(mul24_device(5u, 1u << 24) == 0u);

    if (fails) return 1;
    std::printf("no difference (%lld staging units, %lld products)\n", units, prods);
    return 0;
}
