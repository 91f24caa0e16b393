// stats_spans_replay.cpp -- the frame metrics' launch geometry and lane map replayed on the host (tests/test_gpu_stats_spans.py compiles
// it, host side only): stat_grid and the very functions frame_stats_kernel deals its lanes with (stats_body.h).
//   stats_spans_replay es pitch_elems W H nframes
// prints "gx gy col_groups buf ragged tile_rows", then one line "wave tile col" per lane of the gx workgroups of a frame run, in launch
// order (workgroup 0 lane 0, workgroup 0 lane 1, ...); wave: the wave's place in the run's order of waves.
#include <cstdio>
#include <cstdlib>

#include "stats_body.h"

int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    const int es = atoi(argv[1]), pitch = atoi(argv[2]), W = atoi(argv[3]), H = atoi(argv[4]), n = atoi(argv[5]);
    const amt::StatGrid g = amt::stat_grid(es, pitch, W, H, n);
    const int tile_rows = !g.buf ? amt::kStatTileRowsPlain : es == 1 ? amt::kStatTileRows8 : amt::kStatTileRows;
    printf("%d %d %d %d %d %d\n", g.gx, g.gy, g.col_groups, (int)g.buf, (int)g.ragged, tile_rows);
    for (int b = 0; b < g.gx; ++b)
        for (int t = 0; t < amt::kStatThreads; ++t) {
            const int wg = amt::stat_workgroup(g.gx, b);
            const amt::StatLane sl = amt::stat_lane(g.col_groups, wg * amt::kStatThreads + t);
            printf("%d %d %d\n", wg * (amt::kStatThreads / 64) + (t >> 6), sl.tile, sl.col);
        }
    return 0;
}
