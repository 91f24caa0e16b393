// tile_units_replay.cpp -- CPU replay of the single-pass tile plans (amatsukaze_amd/csrc/eval_tiles.hpp, kTileCutUnits) that the scan's
// one-unit pair kernel runs on (eval_pair1_kernels.hip): a tile stages only the units some window of its pixels reads, one unit per lane,
// taken from the plan's list.  For every such plan:
//   * every mask pixel sits in exactly one slot and the bands are raster-consecutive;
//   * every tile lists at most 64 units; entries from nunits on repeat the last needed unit;
//   * every element of every slot's 5x5 window -- a lane with a pixel or a filler lane -- lies in a listed unit, at the plane offset
//     the window reads, and a pixel's window holds the samples CalcCorrelation5x5 reads (LogoScan.hpp:24-41);
//   * every listed unit is read by the window of some lane that carries a pixel;
//   * units load inside the logo and store at even plane offsets below kTileCap, no two samples in one cell.
// One STATS line per mask carries the figures of the existing cuts beside the single-pass plan's (tests/test_tile_units.py reads it).
//   usage: tile_units_replay            (seeded synthetic masks)
//          tile_units_replay pos.bin    (int32 count, w, h, then count x uint32 (y << 16) | x)
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>

#include "eval_tiles.hpp"

using namespace amt;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// the units of tile t of plan P that the window of a lane with a pixel reads, as tile_unit_word(row, c4)
static std::set<uint32_t> needed_units(const TilePlan& P, size_t t, const std::vector<uint32_t>& pos)
{
    const TileDesc& T = P.tiles[t];
    std::set<uint32_t> need;
    for (int l = 0; l < kTileLanes; ++l) {
        const int m = P.slot_pixel[t * kTileLanes + l];
        if (m < 0) continue;
        const int px = (int)(pos[m] & 0xFFFFu), py = (int)(pos[m] >> 16);
        for (int y = py - 2; y <= py + 2; ++y)
            for (int x = px - 2; x <= px + 2; ++x) need.insert(tile_unit_word(y - T.y0, (x - T.x0) / 4));
    }
    return need;
}

struct CutStats { int tiles = 0, bands = 0; long box = 0, need = 0; int over_box = 0, over_need = 0; long long cost = 0; };
static CutStats stats_of(const TilePlan& P, const std::vector<uint32_t>& pos)
{
    CutStats S;
    S.bands = (int)P.bands.size();
    S.cost = P.model_cost;
    for (size_t t = 0; t < P.tiles.size(); ++t) {
        const TileDesc& T = P.tiles[t];
        if (T.npix <= 0) continue;
        const int box = T.nrows * T.ncol4, need = (int)needed_units(P, t, pos).size();
        ++S.tiles; S.box += box; S.need += need;
        S.over_box += box > kTileLanes; S.over_need += need > kTileLanes;
    }
    return S;
}

static void replay(const char* name, const std::vector<uint32_t>& pos, int w, int h)
{
    const int count = (int)pos.size();
    const TilePlan P = build_tile_plan(pos, count, w, h, kTileCutUnits);
    std::vector<int> seen(count, 0);
    int m_next = 0, max_nunits = 0, at64 = 0, stopped = 0;
    CHECK(P.single_pass, "%s: not a single-pass plan", name);
    CHECK(P.tiles.size() == P.bands.size() * kTileWaves && P.sinfo.size() == P.bands.size() * kTileBandPix &&
          P.units.size() == P.sinfo.size() && P.nunits.size() == P.tiles.size(), "%s: table sizes", name);
    for (size_t b = 0; b < P.bands.size(); ++b) {
        const TileBandDesc& B = P.bands[b];
        CHECK(B.m0 == m_next && B.npix >= 1 && B.npix <= kTileBandPix, "%s: band %zu range", name, b);
        m_next = B.m0 + B.npix;
        std::vector<int> row_seen(kTileBandPix, 0);
        for (int wv = 0; wv < kTileWaves; ++wv) {
            const size_t t = b * kTileWaves + wv;
            const TileDesc& T = P.tiles[t];
            const int nu = P.nunits[t];
            const uint32_t* list = &P.units[t * kTileLanes];
            CHECK(T.npix >= 0 && T.npix <= kTileLanes && T.nrows * T.tp <= kTileCap && T.tp >= 4 * T.ncol4 && (T.tp & 1) == 0 && (T.x0 & 1) == 0,
                  "%s: band %zu tile %d geometry", name, b, wv);
            CHECK(nu >= 0 && nu <= kTileLanes && (nu > 0) == (T.npix > 0), "%s: band %zu tile %d lists %d units for %d pixels", name, b, wv, nu, T.npix);
            max_nunits = std::max(max_nunits, nu);
            at64 += nu == kTileLanes;
            // staging, as the kernel's lanes do it: lane l takes entry l
            std::vector<int> cell(kTileCap, -1);
            for (int l = 0; l < kTileLanes; ++l) {
                if (l >= nu) CHECK(list[l] == list[nu > 0 ? nu - 1 : 0] && (nu > 0 || list[l] == tile_unit_word(0, 0)), "%s: band %zu tile %d entry %d past the list", name, b, wv, l);
                if (l > 0 && l < nu) CHECK(list[l] > list[l - 1], "%s: band %zu tile %d list not in raster order", name, b, wv);
                const TileUnit U = tile_unit_listed(T, list[l], w);
                CHECK(U.y >= 0 && U.y < h && U.xs >= 0 && U.xs + 3 < w && (U.xs & 1) == 0, "%s: unit reads outside the logo (y %d xs %d)", name, U.y, U.xs);
                CHECK(U.lds >= 0 && U.lds + 3 < kTileCap && (U.lds & 1) == 0, "%s: unit store outside the plane (%d)", name, U.lds);
                if (T.npix > 0) CHECK((int)(list[l] >> 8) < T.nrows && (int)(list[l] & 0xFFu) < T.ncol4, "%s: band %zu tile %d unit outside the box", name, b, wv);
                for (int j = 0; j < 4 && U.lds >= 0 && U.lds + j < kTileCap; ++j) {
                    const int coord = U.y * 65536 + U.xs + j;
                    CHECK(cell[U.lds + j] == -1 || cell[U.lds + j] == coord, "%s: two samples in one LDS cell", name);
                    cell[U.lds + j] = coord;
                }
            }
            const std::set<uint32_t> need = needed_units(P, t, pos);
            CHECK((int)need.size() == nu, "%s: band %zu tile %d: %zu units are read, %d listed", name, b, wv, need.size(), nu);
            for (int l = 0; l < nu; ++l) CHECK(need.count(list[l]) == 1, "%s: band %zu tile %d lists a unit no pixel's window reads", name, b, wv);
            int nvalid = 0, xlast = -1, mlast = -1;
            for (int l = 0; l < kTileLanes; ++l) {
                const size_t slot = t * kTileLanes + l;
                const uint32_t si = P.sinfo[slot];
                const bool valid = (si >> 31) != 0;
                const int m = P.slot_pixel[slot];
                CHECK(valid == (m >= 0), "%s: slot validity", name);
                nvalid += valid;
                const int woff = (int)(si & 0xFFFu), ridx = (int)((si >> 12) & 0xFFFu);
                CHECK(woff + 4 * std::max(T.tp, 4) + 4 < kTileCap, "%s: window past the plane", name);
                if (T.npix == 0) continue;                      // (a wave without a tile: nothing is written out, nothing is staged for it)
                for (int r = 0; r < 5; ++r)
                    for (int c = 0; c < 5; ++c) {
                        const int at = woff + r * T.tp + c;
                        CHECK(at < kTileCap && cell[at] != -1, "%s: band %zu tile %d lane %d window (%d,%d) reads a cell no listed unit stages", name, b, wv, l, r, c);
                    }
                if (!valid) continue;
                CHECK(m >= B.m0 && m < B.m0 + B.npix && ridx == m - B.m0, "%s: score row index", name);
                ++seen[m];
                ++row_seen[ridx];
                const int px = (int)(pos[m] & 0xFFFFu), py = (int)(pos[m] >> 16);
                if (px > xlast || (px == xlast && m > mlast)) { xlast = px; mlast = m; }
                for (int r = 0; r < 5; ++r)
                    for (int c = 0; c < 5; ++c) {
                        const int at = woff + r * T.tp + c;
                        CHECK(at < kTileCap && cell[at] == (py - 2 + r) * 65536 + (px - 2 + c), "%s: band %zu tile %d lane %d window (%d,%d) reads the wrong sample",
                              name, b, wv, l, r, c);
                    }
            }
            CHECK(nvalid == T.npix, "%s: band %zu tile %d: %d lanes carry a pixel, the tile says %d", name, b, wv, nvalid, T.npix);
            // a tile that stopped growing at the unit limit: the band's next pixel by column would have made it 65 units or more
            if (T.npix > 0 && T.npix < kTileLanes) {
                int xn = 1 << 30, mn = -1;
                for (int m = B.m0; m < B.m0 + B.npix; ++m) {
                    const int x = (int)(pos[m] & 0xFFFFu);
                    if ((x > xlast || (x == xlast && m > mlast)) && (x < xn || (x == xn && m < mn))) { xn = x; mn = m; }
                }
                if (mn >= 0) {
                    std::set<uint32_t> grown;                    // (keyed by the logo row: the next pixel's window may start above the tile)
                    for (uint32_t k : need) grown.insert((((k >> 8) + (uint32_t)T.y0) << 8) | (k & 0xFFu));
                    const int px = xn, py = (int)(pos[mn] >> 16);
                    for (int y = py - 2; y <= py + 2; ++y)
                        for (int x = px - 2; x <= px + 2; ++x) grown.insert(((uint32_t)y << 8) | (uint32_t)((x - T.x0) / 4));
                    stopped += grown.size() > (size_t)kTileLanes;
                }
            }
        }
        for (int i = 0; i < B.npix; ++i) CHECK(row_seen[i] == 1, "%s: band %zu row slot %d written %d times", name, b, i, row_seen[i]);
    }
    CHECK(m_next == count, "%s: bands cover %d of %d pixels", name, m_next, count);
    for (int m = 0; m < count; ++m) CHECK(seen[m] == 1, "%s: pixel %d evaluated %d times", name, m, seen[m]);

    // the existing cuts beside it, and the engine's choice for an engine of this logo alone
    const TilePlan coarse = build_tile_plan(pos, count, w, h, kTileCutCoarse), fine = build_tile_plan(pos, count, w, h, kTileCutFine);
    const TilePlan best = build_tile_plan(pos, count, w, h, kTileCutBest);
    CHECK(!coarse.single_pass && !fine.single_pass && !best.single_pass && best.units.empty(), "%s: an existing cut became a single-pass plan", name);
    CHECK(best.model_cost == std::min(coarse.model_cost, fine.model_cost), "%s: best cut", name);
    const CutStats C = stats_of(coarse, pos), F = stats_of(fine, pos), U = stats_of(P, pos);
    CHECK(U.over_need == 0 && U.cost == P.model_cost, "%s: single-pass plan with a two-pass tile", name);
    const bool chosen = tile_plans_single_pass(std::vector<TilePlan>{best}, std::vector<TilePlan>{P});
    auto pr = [](const char* tag, const CutStats& S) {
        printf(" %s_tiles=%d %s_bands=%d %s_box=%.2f %s_need=%.2f %s_over_box=%.1f %s_over_need=%.1f %s_cost=%lld", tag, S.tiles, tag, S.bands, tag,
               S.tiles ? (double)S.box / S.tiles : 0.0, tag, S.tiles ? (double)S.need / S.tiles : 0.0, tag, S.tiles ? 100.0 * S.over_box / S.tiles : 0.0,
               tag, S.tiles ? 100.0 * S.over_need / S.tiles : 0.0, tag, S.cost);
    };
    printf("STATS px=%d", count);
    pr("coarse", C); pr("fine", F); pr("units", U);
    printf(" max_nunits=%d tiles_at_64=%d tiles_stopped_by_units=%d single_pass=%d name=%s\n", max_nunits, at64, stopped, chosen ? 1 : 0, name);
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
        replay(argv[1], pos, hdr[1], hdr[2]);
    } else {
        std::mt19937 rng(20240611);
        struct Case { const char* name; int w, h; double density; int kind; };
        const Case cases[] = {
            {"random-35%-256x128", 256, 128, 0.35, 0}, {"random-2%-256x128", 256, 128, 0.02, 0}, {"full-256x128", 256, 128, 1.0, 0},
            {"strokes-256x128", 256, 128, 0.0, 1}, {"columns-256x128", 256, 128, 0.0, 2}, {"wide-1022x40", 1022, 40, 0.3, 0},
            {"tall-22x400", 22, 400, 0.5, 0}, {"tiny-6x6", 6, 6, 1.0, 0}, {"narrow-6x200", 6, 200, 1.0, 0}, {"w%4==2-66x50", 66, 50, 0.4, 0},
            {"one-pixel", 64, 64, 0.0, 3}, {"empty", 64, 64, 0.0, 4}, {"diagonal-300x300", 300, 300, 0.0, 5}, {"full-64x24", 64, 24, 1.0, 0},
            {"random-10%-130x20", 130, 20, 0.1, 0}, {"random-60%-90x33", 90, 33, 0.6, 0},
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
                    }
                    mask[x + (size_t)y * c.w] = on;
                }
            replay(c.name, from_mask(mask, c.w, c.h), c.w, c.h);
        }
    }
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
