// pair_shape_replay.cpp -- CPU replay of the scan pair kernel's shape choice (amatsukaze_amd/csrc/eval_tiles.hpp tile_pair_shape) and of the
// plans its second shape walks: single-pass plans (kTileCutUnits) of kPairDuoWaves tiles per band, built through build_tile_plan's
// trailing wave-count argument.  For every mask:
//   * every cut built with the argument at kTileWaves is byte for byte the plan built without it;
//   * at kPairDuoWaves every mask pixel sits in exactly one slot, the slots of a band cover its raster-consecutive pixels once each at
//     their raster index (the sum's order is the reference's), a band has at most kPairDuoWaves tiles and 64 times as many pixels, a tile
//     lists at most 64 needed units, and every window lies inside its tile's plane.
// Then the chooser's verdict for the masks taken together as one engine's logo list, one CHOICE line; one PLAN line per mask.
//   usage: pair_shape_replay [--lds BYTES]               (seeded synthetic masks, each an engine of its own)
//          pair_shape_replay [--lds BYTES] pos.bin ...   (int32 count, w, h, then count x uint32 (y << 16) | x; the files are ONE list)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "eval_tiles.hpp"

using namespace amt;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

constexpr int kRowPad = 36;                 // kEvalScorePad (eval_plan.h, a HIP header)

template <typename T> static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static bool same_plan(const TilePlan& a, const TilePlan& b)
{
    return same_bytes(a.bands, b.bands) && same_bytes(a.tiles, b.tiles) && same_bytes(a.sinfo, b.sinfo) && same_bytes(a.slot_pixel, b.slot_pixel) &&
           same_bytes(a.units, b.units) && same_bytes(a.nunits, b.nunits) && a.model_cost == b.model_cost && a.work_cost == b.work_cost &&
           a.single_pass == b.single_pass && a.waves == b.waves;
}

struct Mask { std::string name; std::vector<uint32_t> pos; int w, h; };

static void check_default_argument(const Mask& M)
{
    const int count = (int)M.pos.size();
    const TileCut cuts[] = {kTileCutCoarse, kTileCutFine, kTileCutBest, kTileCutUnits};
    for (const TileCut cut : cuts) {
        const TilePlan a = build_tile_plan(M.pos, count, M.w, M.h, cut), b = build_tile_plan(M.pos, count, M.w, M.h, cut, kTileWaves);
        CHECK(same_plan(a, b) && a.waves == kTileWaves, "%s: cut %d differs with the wave count passed", M.name.c_str(), (int)cut);
        CHECK(a.tiles.size() == a.bands.size() * kTileWaves && a.sinfo.size() == a.bands.size() * kTileBandPix, "%s: cut %d strides", M.name.c_str(), (int)cut);
    }
}

static void check_plan(const Mask& M, const TilePlan& P, int nw)
{
    const char* name = M.name.c_str();
    const int count = (int)M.pos.size(), band_pix = nw * kTileLanes;
    std::vector<int> seen(count, 0);
    int m_next = 0;
    long long work = 0;
    CHECK(P.single_pass && P.waves == nw, "%s: not a single-pass plan of %d waves", name, nw);
    CHECK(P.tiles.size() == P.bands.size() * nw && P.sinfo.size() == P.bands.size() * band_pix && P.slot_pixel.size() == P.sinfo.size() &&
          P.units.size() == P.sinfo.size() && P.nunits.size() == P.tiles.size(), "%s: table sizes", name);
    if (failures) return;
    for (size_t b = 0; b < P.bands.size(); ++b) {
        const TileBandDesc& B = P.bands[b];
        CHECK(B.m0 == m_next && B.npix >= 1 && B.npix <= band_pix, "%s: band %zu range", name, b);
        m_next = B.m0 + B.npix;
        std::vector<int> row_seen(band_pix, 0);
        for (int wv = 0; wv < nw; ++wv) {
            const size_t t = b * nw + wv;
            const TileDesc& T = P.tiles[t];
            CHECK(T.npix >= 0 && T.npix <= kTileLanes && T.nrows * T.tp <= kTileCap && T.tp >= 4 * T.ncol4 && (T.tp & 1) == 0 && (T.x0 & 1) == 0,
                  "%s: band %zu tile %d geometry", name, b, wv);
            CHECK(P.nunits[t] >= 0 && P.nunits[t] <= kTileLanes && (P.nunits[t] > 0) == (T.npix > 0), "%s: band %zu tile %d lists %d units", name, b, wv, P.nunits[t]);
            work += T.npix > 0 ? 162 : 0;
            int nvalid = 0;
            for (int l = 0; l < kTileLanes; ++l) {
                const size_t slot = t * kTileLanes + l;
                const uint32_t si = P.sinfo[slot];
                const bool valid = (si >> 31) != 0;
                const int m = P.slot_pixel[slot];
                const int woff = (int)(si & 0xFFFu), ridx = (int)((si >> 12) & 0xFFFu);
                CHECK(valid == (m >= 0), "%s: slot validity", name);
                CHECK(woff + 4 * std::max(T.tp, 4) + 4 < kTileCap, "%s: window past the plane", name);
                // a listed unit stages inside the plane and loads inside the logo
                const TileUnit U = tile_unit_listed(T, P.units[slot], M.w);
                CHECK(U.y >= 0 && U.y < M.h && U.xs >= 0 && U.xs + 3 < M.w && U.lds >= 0 && U.lds + 3 < kTileCap, "%s: band %zu tile %d unit outside", name, b, wv);
                if (!valid) continue;
                ++nvalid;
                CHECK(m >= B.m0 && m < B.m0 + B.npix && ridx == m - B.m0, "%s: band %zu tile %d lane %d: pixel %d at row index %d", name, b, wv, l, m, ridx);
                if (m < 0 || m >= count) continue;
                ++seen[m];
                if (ridx < band_pix) ++row_seen[ridx];
                // the window's 25 elements lie inside the tile's box, at the offsets the pixel's position gives
                const int px = (int)(M.pos[m] & 0xFFFFu), py = (int)(M.pos[m] >> 16);
                CHECK(woff == (py - 2 - T.y0) * T.tp + (px - 2 - T.x0), "%s: window offset", name);
                CHECK(px - 2 >= T.x0 && px + 2 < T.x0 + 4 * T.ncol4 && py - 2 >= T.y0 && py + 2 < T.y0 + T.nrows, "%s: band %zu tile %d window outside its tile", name, b, wv);
            }
            CHECK(nvalid == T.npix, "%s: band %zu tile %d: %d lanes carry a pixel, the tile says %d", name, b, wv, nvalid, T.npix);
        }
        for (int i = 0; i < B.npix; ++i) CHECK(row_seen[i] == 1, "%s: band %zu row slot %d written %d times", name, b, i, row_seen[i]);
    }
    CHECK(m_next == count, "%s: bands cover %d of %d pixels", name, m_next, count);
    for (int m = 0; m < count; ++m) CHECK(seen[m] == 1, "%s: pixel %d evaluated %d times", name, m, seen[m]);
    CHECK(work == P.work_cost, "%s: work cost %lld, the plan says %lld", name, work, P.work_cost);
}

// the engine's choice (EvalEngine::ensure_tiles) for the masks as one logo list
static void choose(const std::vector<Mask>& list, size_t lds)
{
    std::vector<TilePlan> best, units, duo;
    for (const Mask& M : list) {
        const int count = (int)M.pos.size();
        best.push_back(build_tile_plan(M.pos, count, M.w, M.h, kTileCutBest));
        units.push_back(build_tile_plan(M.pos, count, M.w, M.h, kTileCutUnits));
        duo.push_back(build_tile_plan(M.pos, count, M.w, M.h, kTileCutUnits, kPairDuoWaves));
        check_plan(M, duo.back(), kPairDuoWaves);
        const TilePlan& D = duo.back();
        std::string per_band;
        for (size_t b = 0; b < D.bands.size(); ++b) {
            int n = 0;
            for (int wv = 0; wv < D.waves; ++wv) n += D.tiles[b * D.waves + wv].npix > 0;
            per_band += (b ? "," : "") + std::to_string(n);
        }
        printf("PLAN px=%d best_cost=%lld units_cost=%lld duo_cost=%lld duo_work=%lld duo_bands=%zu duo_tiles_per_band=%s name=%s\n", count, best.back().model_cost,
               units.back().model_cost, D.model_cost, D.work_cost, D.bands.size(), per_band.empty() ? "-" : per_band.c_str(), M.name.c_str());
    }
    const PairShape S = tile_pair_shape(best, units, duo, lds, kRowPad);
    const bool single = tile_plans_single_pass(best, units);
    CHECK((S.duo && S.waves == kPairDuoWaves && S.frames == kPairDuoFrames) || (!S.duo && S.waves == kTileWaves && S.frames == kTileMaxFrames), "shape %d / %d / %d", S.waves, S.frames, (int)S.duo);
    if (S.duo) CHECK(tile_pair_lds_bytes(S.waves, S.frames, kRowPad) <= lds, "the duo shape's LDS does not fit %zu", lds);
    printf("CHOICE logos=%zu waves=%d frames=%d duo=%d one_unit=%d lds=%zu lds_limit=%zu\n", list.size(), S.waves, S.frames, (int)S.duo, (S.duo || single) ? 1 : 0,
           tile_pair_lds_bytes(S.waves, S.frames, kRowPad), lds);
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
    size_t lds = 160 * 1024;
    int a = 1;
    if (a + 1 < argc && !strcmp(argv[a], "--lds")) { lds = (size_t)atoll(argv[a + 1]); a += 2; }
    if (a < argc) {
        std::vector<Mask> list;
        for (; a < argc; ++a) {
            FILE* f = fopen(argv[a], "rb");
            int hdr[3];
            if (!f || fread(hdr, 4, 3, f) != 3 || hdr[0] < 0) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
            Mask M{argv[a], std::vector<uint32_t>((size_t)hdr[0]), hdr[1], hdr[2]};
            if (fread(M.pos.data(), 4, M.pos.size(), f) != M.pos.size()) return 2;
            fclose(f);
            check_default_argument(M);
            list.push_back(M);
        }
        choose(list, lds);
    } else {
        std::mt19937 rng(20240611);
        struct Case { const char* name; int w, h; double density; int kind; };
        const Case cases[] = {
            {"random-35%-256x128", 256, 128, 0.35, 0}, {"random-2%-256x128", 256, 128, 0.02, 0}, {"full-256x128", 256, 128, 1.0, 0},
            {"strokes-256x128", 256, 128, 0.0, 1}, {"columns-256x128", 256, 128, 0.0, 2}, {"wide-1022x40", 1022, 40, 0.3, 0},
            {"tall-22x400", 22, 400, 0.5, 0}, {"tiny-6x6", 6, 6, 1.0, 0}, {"narrow-6x200", 6, 200, 1.0, 0}, {"w%4==2-66x50", 66, 50, 0.4, 0},
            {"one-pixel", 64, 64, 0.0, 3}, {"diagonal-300x300", 300, 300, 0.0, 5}, {"full-64x24", 64, 24, 1.0, 0},
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
                    case 5: on = (x - y) % 97 == 0 || x == y; break;
                    }
                    mask[x + (size_t)y * c.w] = on;
                }
            const Mask M{c.name, from_mask(mask, c.w, c.h), c.w, c.h};
            check_default_argument(M);
            choose(std::vector<Mask>{M}, lds);
        }
    }
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
