// tile_cut_test.cpp -- the band cutters of amatsukaze_amd/csrc/eval_tiles.hpp (TileCut): every cut must give a plan the tile kernels can
// walk -- bands of raster-consecutive mask pixels, at most kTileWaves tiles each, every mask pixel evaluated once at its raster
// position, every 5x5 window inside its tile and reading the samples CalcCorrelation5x5 reads (LogoScan.hpp:24-41) -- and the cut the
// scan kernel uses (kTileCutBest) must never have a higher modelled critical path than the coarse one.
//   usage: tile_cut_test                      (built-in synthetic masks)
//          tile_cut_test pos.bin [max_bands]  (int32 count, w, h, then count x uint32 (y << 16) | x; max_bands: bound on the best cut's bands)
// Prints per mask: bands and modelled critical path of the coarse, the fine and the best cut.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "eval_tiles.hpp"

using namespace amt;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// the modelled critical path, recomputed from the tiles alone: wave v runs on SIMD v % 4
static long long model_cost(const TilePlan& P)
{
    long long total = 0;
    for (size_t b = 0; b < P.bands.size(); ++b) {
        int load[4] = {0, 0, 0, 0};
        for (int wv = 0; wv < kTileWaves; ++wv) {
            const TileDesc& T = P.tiles[b * kTileWaves + wv];
            if (T.npix > 0) load[wv % 4] += 131 + 31 * (T.nrows * T.ncol4 > kTileLanes ? 2 : 1);
        }
        total += *std::max_element(load, load + 4);
    }
    return total;
}

static void check_plan(const char* name, const char* cut, const TilePlan& P, const std::vector<uint32_t>& pos, int w, int h)
{
    const int count = (int)pos.size();
    std::vector<int> seen(count, 0);
    int m_next = 0;
    CHECK(P.tiles.size() == P.bands.size() * kTileWaves && P.sinfo.size() == P.bands.size() * kTileBandPix && P.slot_pixel.size() == P.sinfo.size(),
          "%s %s: table sizes", name, cut);
    CHECK(P.model_cost == model_cost(P), "%s %s: the plan's modelled cost %lld is not that of its tiles (%lld)", name, cut, P.model_cost, model_cost(P));
    for (size_t b = 0; b < P.bands.size(); ++b) {
        const TileBandDesc& B = P.bands[b];
        CHECK(B.m0 == m_next && B.npix >= 1 && B.npix <= kTileBandPix, "%s %s: band %zu range", name, cut, b);
        m_next = B.m0 + B.npix;
        std::vector<int> row_seen(kTileBandPix, 0);
        for (int wv = 0; wv < kTileWaves; ++wv) {
            const TileDesc& T = P.tiles[b * kTileWaves + wv];
            CHECK(T.npix >= 0 && T.npix <= kTileLanes && T.nrows * T.tp <= kTileCap && T.tp >= 4 * T.ncol4 && (T.tp & 1) == 0 && (T.x0 & 1) == 0 &&
                  T.nrows * T.ncol4 <= kTileLanes * kTileUnits, "%s %s: band %zu tile %d geometry", name, cut, b, wv);
            std::vector<int> cell(kTileCap, -1);                   // staging, as the kernels' lanes do it
            for (int u = 0; u < kTileLanes * kTileUnits; ++u) {
                const TileUnit U = tile_unit(T, u, w);
                CHECK(U.y >= 0 && U.y < h && U.xs >= 0 && U.xs + 3 < w && U.lds >= 0 && U.lds + 3 < kTileCap, "%s %s: unit outside the logo or the plane", name, cut);
                if (U.lds < 0 || U.lds + 3 >= kTileCap) continue;
                for (int j = 0; j < 4; ++j) {
                    const int coord = U.y * 65536 + U.xs + j;
                    CHECK(cell[U.lds + j] == -1 || cell[U.lds + j] == coord, "%s %s: two samples in one LDS cell", name, cut);
                    cell[U.lds + j] = coord;
                }
            }
            int nvalid = 0;
            for (int l = 0; l < kTileLanes; ++l) {
                const size_t slot = (b * kTileWaves + wv) * kTileLanes + l;
                const uint32_t si = P.sinfo[slot];
                const int m = P.slot_pixel[slot];
                const int woff = (int)(si & 0xFFFu), ridx = (int)((si >> 12) & 0xFFFu);
                CHECK(((si >> 31) != 0) == (m >= 0), "%s %s: slot validity", name, cut);
                CHECK(woff + 4 * std::max(T.tp, 4) + 4 < kTileCap, "%s %s: window outside the plane", name, cut);
                if (m < 0) continue;
                ++nvalid;
                CHECK(m >= B.m0 && m < B.m0 + B.npix && ridx == m - B.m0, "%s %s: score row index", name, cut);
                if (m < 0 || m >= count) continue;
                ++seen[m];
                ++row_seen[ridx];
                const int px = (int)(pos[m] & 0xFFFFu), py = (int)(pos[m] >> 16);
                for (int r = 0; r < 5; ++r)
                    for (int c = 0; c < 5; ++c) {
                        const int at = woff + r * T.tp + c;
                        CHECK(at < kTileCap && cell[at] == (py - 2 + r) * 65536 + (px - 2 + c), "%s %s: band %zu tile %d lane %d window (%d,%d) reads the wrong sample",
                              name, cut, b, wv, l, r, c);
                    }
            }
            CHECK(nvalid == T.npix, "%s %s: band %zu tile %d: %d lanes carry a pixel, the tile says %d", name, cut, b, wv, nvalid, T.npix);
        }
        for (int i = 0; i < B.npix; ++i) CHECK(row_seen[i] == 1, "%s %s: band %zu row slot %d written %d times", name, cut, b, i, row_seen[i]);
    }
    CHECK(m_next == count, "%s %s: bands cover %d of %d pixels", name, cut, m_next, count);
    for (int m = 0; m < count; ++m) CHECK(seen[m] == 1, "%s %s: pixel %d evaluated %d times", name, cut, m, seen[m]);
}

static void run(const char* name, const std::vector<uint32_t>& pos, int w, int h, int max_bands)
{
    const int count = (int)pos.size();
    const TilePlan coarse = build_tile_plan(pos, count, w, h), fine = build_tile_plan(pos, count, w, h, kTileCutFine),
                   best = build_tile_plan(pos, count, w, h, kTileCutBest);
    check_plan(name, "coarse", coarse, pos, w, h);
    check_plan(name, "fine", fine, pos, w, h);
    check_plan(name, "best", best, pos, w, h);
    // the default cut is the coarse one (the linear analysis kernel's summation order depends on it)
    const TilePlan dflt = build_tile_plan(pos, count, w, h, kTileCutCoarse);
    CHECK(dflt.sinfo == coarse.sinfo && dflt.slot_pixel == coarse.slot_pixel && dflt.bands.size() == coarse.bands.size(), "%s: the default cut is not the coarse one", name);
    CHECK(best.model_cost <= coarse.model_cost, "%s: the best cut's modelled critical path %lld is above the coarse cut's %lld", name, best.model_cost, coarse.model_cost);
    CHECK(best.model_cost == std::min(coarse.model_cost, fine.model_cost), "%s: the best cut is neither of the two", name);
    CHECK(best.bands.size() <= coarse.bands.size() || best.model_cost < coarse.model_cost, "%s: more bands without a lower cost", name);
    if (max_bands > 0) CHECK((int)best.bands.size() <= max_bands, "%s: the best cut has %zu bands, expected at most %d", name, best.bands.size(), max_bands);
    printf("%-28s %6d px  bands %3zu / %3zu / %3zu  modelled critical path %7lld / %7lld / %7lld  (coarse / fine / best)\n", name, count, coarse.bands.size(),
           fine.bands.size(), best.bands.size(), coarse.model_cost, fine.model_cost, best.model_cost);
}

static std::vector<uint32_t> from_mask(const std::vector<uint8_t>& mask, int w, int h)
{
    std::vector<uint32_t> pos;
    for (int y = 2; y < h - 2; ++y)
        for (int x = 2; x < w - 2; ++x)
            if (mask[x + y * w]) pos.push_back(((uint32_t)y << 16) | (uint32_t)x);
    return pos;
}

int main(int argc, char** argv)
{
    if (argc > 1) {
        FILE* f = fopen(argv[1], "rb");
        int hdr[3];
        if (!f || fread(hdr, 4, 3, f) != 3) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        std::vector<uint32_t> pos(hdr[0]);
        if (fread(pos.data(), 4, pos.size(), f) != pos.size()) return 2;
        fclose(f);
        run(argv[1], pos, hdr[1], hdr[2], argc > 2 ? atoi(argv[2]) : 0);
    } else {
        // the synthetic masks of eval_tiles_test.cpp, plus a ragged right edge (w % 4 != 0 with pixels in the last columns) and a one-tile logo
        std::mt19937 rng(12345);
        struct Case { const char* name; int w, h; double density; int kind; };
        const Case cases[] = {
            {"random 35% 256x128", 256, 128, 0.35, 0}, {"random 2% 256x128", 256, 128, 0.02, 0}, {"full 256x128", 256, 128, 1.0, 0},
            {"strokes 256x128", 256, 128, 0.0, 1}, {"columns 256x128", 256, 128, 0.0, 2}, {"wide 1022x40", 1022, 40, 0.3, 0},
            {"tall 22x400", 22, 400, 0.5, 0}, {"tiny 6x6", 6, 6, 1.0, 0}, {"narrow 6x200", 6, 200, 1.0, 0}, {"w%4==2 66x50", 66, 50, 0.4, 0},
            {"one pixel", 64, 64, 0.0, 3}, {"empty", 64, 64, 0.0, 4}, {"diagonal 300x300", 300, 300, 0.0, 5},
            {"ragged edge 70x60", 70, 60, 0.0, 6}, {"one tile 12x10", 12, 10, 1.0, 0},
        };
        for (const Case& c : cases) {
            std::vector<uint8_t> mask((size_t)c.w * c.h, 0);
            std::uniform_real_distribution<double> U(0, 1);
            for (int y = 0; y < c.h; ++y)
                for (int x = 0; x < c.w; ++x) {
                    bool on = false;
                    switch (c.kind) {
                    case 0: on = U(rng) < c.density; break;
                    case 1: on = ((x / 7 + y / 5) % 3 == 0) && U(rng) < 0.8; break;       // text-like strokes
                    case 2: on = x % 37 < 3; break;
                    case 3: on = x == 31 && y == 17; break;
                    case 4: on = false; break;
                    case 5: on = (x - y) % 97 == 0 || x == y; break;
                    case 6: on = x >= c.w - 8; break;                                     // everything at the right edge
                    }
                    mask[x + (size_t)y * c.w] = on;
                }
            run(c.name, from_mask(mask, c.w, c.h), c.w, c.h, 0);
        }
    }
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
