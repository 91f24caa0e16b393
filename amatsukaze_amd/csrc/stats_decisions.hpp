// stats_decisions.hpp -- host decisions on the whole-frame metrics (self-specified):
// scene changes (what the reference obtains from chapter_exe's "SCPos:" lines, CMAnalyze.hpp:411-439) and
// the per-frame cadence class that the KFM analysis passes would leave in *.duration.txt
// (FilteredSource.hpp:265-269,637-676).  Integer arithmetic only.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace amt {

enum Cadence : uint8_t { kCadence60i = 0, kCadence24p = 1, kCadence30p = 2 };

std::vector<int> scene_changes(const uint64_t* metrics, int nframes, int width, int height);
void classify_cadence(const uint64_t* metrics, int nframes, int width, int height, uint8_t* cadence, uint8_t* phase);
// durations in 60p ticks of the clip AMTDecimate wraps: 60i frame -> 1,1; 30p -> 2; a full 3:2 cycle -> 2,3,2,3
std::vector<int> cadence_durations(const uint8_t* cadence, const uint8_t* phase, int nframes);
// The pictures that go with those durations (self-specified), one entry per output frame in the order of
// cadence_durations and with its ticks: a full 3:2 cycle at n -> WEAVE(n, n), WEAVE(n+1, n+1), WEAVE(top n+3, bottom n+2), WEAVE(n+4, n+4);
// a 60i frame -> BOB_TOP(n), BOB_BOTTOM(n); anything else -> WEAVE(n, n).  Source frame numbers are absolute.  The layout is
// AmtGpuRenderFrame's (amt_gpu.h)
enum RenderKind : int32_t { kRenderWeave = 0, kRenderBobTop = 1, kRenderBobBottom = 2 };
struct RenderFrame { int32_t kind, top, bottom, ticks; };
std::vector<RenderFrame> cadence_render_plan(const uint8_t* cadence, const uint8_t* phase, int nframes);
// Mute sections from the audio levels (4 uint64 per video frame: AMTGPU_AL_*; self-specified): a frame is silent
// when its PEAK is at most mute_level or it owns no samples at all (COUNT 0); a section is a maximal run of at least min_frames silent
// frames, inclusive [first, last]
std::vector<std::pair<int, int>> mute_sections(const uint64_t* levels, int nframes, int mute_level, int min_frames);

} // namespace amt
