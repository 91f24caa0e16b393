// amt_gpu_audio.hip -- C ABI part 4: per-video-frame audio levels (self-specified), the mute sections decided
// from them and chapter_exe's output file with its "mute" lines.
#include "build_knobs.h"
#include "../../include/amt_gpu.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "api_common.hpp"
#include "stats_decisions.hpp"

using namespace amt;

static_assert(AMTGPU_AL_WORDS == kAudioLevelWords, "the record of the ABI is the kernel's");

struct AmtGpuAudioLevels {
    AmtGpuContext* ctx;
    AudioTimeline t;                        // num_samples, sample_rate * fps_den, fps_num, channels
    DevBuf<int16_t> dPcm;                   // amtgpu_audiolevels_amts: the chunk's PCM and records
    DevBuf<unsigned long long> dOut;
    std::vector<int16_t> host;
};

namespace {
constexpr int kAmtsChunkFrames = 4096;      // video frames per chunk of amtgpu_audiolevels_amts: 26 MB of 48 kHz stereo at 29.97 fps

// b(frame) of the span rule; -1 where it does not fit 63 bits
int64_t frame_start(const AudioTimeline& t, int64_t frame)
{
    if (frame < 0) return -1;
    const __int128 v = (__int128)frame * t.step_num / t.fps_num, top = (__int128)frame * t.step_num;
    return top > (__int128)INT64_MAX || v > (__int128)INT64_MAX ? -1 : (int64_t)v;
}

// the sample-frames a batch needs: [lo, hi) (empty when all of it lies behind the timeline)
struct Cover { int64_t lo, hi; };
Cover batch_cover(const AmtGpuAudioLevels* al, int first_frame, int nframes)
{
    if (first_frame < 0 || nframes < 0) throw std::runtime_error("[AudioLevels] negative first frame or frame count");
    if ((int64_t)first_frame + nframes > INT32_MAX) throw std::runtime_error("[AudioLevels] frame range beyond 2^31 frames");
    const int64_t lo = frame_start(al->t, first_frame), end = frame_start(al->t, (int64_t)first_frame + nframes);
    if (lo < 0 || end < 0) throw std::runtime_error("[AudioLevels] frame range beyond what 64-bit sample positions hold");
    const int64_t hi = std::min(end, (int64_t)al->t.num_samples);
    return Cover{std::min(lo, hi), hi};
}

void levels_batch(AmtGpuAudioLevels* al, const int16_t* d_pcm, int64_t pcm_first, int64_t pcm_count, int first_frame, int nframes,
                  uint64_t* d_out)
{
    const Cover c = batch_cover(al, first_frame, nframes);
    if (nframes == 0) return;
    if (!d_out) throw std::runtime_error("[AudioLevels] null output pointer");
    if (c.hi > c.lo) {
        if (!d_pcm || (uintptr_t)d_pcm % sizeof(int16_t)) throw std::runtime_error("[AudioLevels] PCM pointer null or not aligned to 2 bytes");
        if (pcm_first < 0 || pcm_count < 0 || pcm_first > c.lo || pcm_count < c.hi - pcm_first)
            throw std::runtime_error("[AudioLevels] the PCM range [" + std::to_string(pcm_first) + ", " + std::to_string(pcm_first) + " + " +
                                     std::to_string(pcm_count) + ") does not cover the frames' sample-frames [" + std::to_string(c.lo) + ", " +
                                     std::to_string(c.hi) + ")");
    }
    al->ctx->bind();
    const int sp = al->ctx->prof_begin("audio_levels_kernel");
    AMT_HIP(launch_audio_levels(al->ctx->stream, d_pcm, pcm_first, al->t, first_frame, nframes, (unsigned long long*)d_out));
    al->ctx->prof_end(sp);
}
} // namespace

extern "C" {

AmtGpuAudioLevels* amtgpu_audiolevels_create(AmtGpuContext* c, int sample_rate, int channels, int fps_num, int fps_den, int64_t num_samples)
{
    AmtGpuAudioLevels* al = nullptr;
    guard(c, [&] {
        if (!c) throw std::runtime_error("no context");
        if (sample_rate <= 0) throw std::runtime_error("[AudioLevels] sample_rate must be positive");
        if (channels < 1 || channels > 8) throw std::runtime_error("[AudioLevels] channels must be 1..8");
        if (fps_num <= 0 || fps_den <= 0) throw std::runtime_error("[AudioLevels] fps_num and fps_den must be positive");
        if (num_samples < 0 || num_samples > INT64_MAX / (8 * (int64_t)sizeof(int16_t))) throw std::runtime_error("[AudioLevels] num_samples out of range");
        al = new AmtGpuAudioLevels{c, AudioTimeline{num_samples, (long long)sample_rate * fps_den, fps_num, channels}};
    });
    return al;
}
void amtgpu_audiolevels_destroy(AmtGpuAudioLevels* al) { delete al; }

int64_t amtgpu_audiolevels_frame_start(const AmtGpuAudioLevels* al, int64_t frame) { return al ? frame_start(al->t, frame) : -1; }

int amtgpu_audiolevels_batch(AmtGpuAudioLevels* al, const int16_t* d_pcm, int64_t pcm_first, int64_t pcm_count, int first_frame, int nframes,
                             uint64_t* d_out)
{
    if (!al) return 0;
    return guard(al->ctx, [&] { levels_batch(al, d_pcm, pcm_first, pcm_count, first_frame, nframes, d_out); });
}

int amtgpu_audiolevels_amts(AmtGpuAudioLevels* al, const AmtGpuAmtsFile* a, const char* wavepath, int first_frame, int nframes, uint64_t* h_out)
{
    if (!al) return 0;
    return guard(al->ctx, [&] {
        AmtGpuContext* c = al->ctx;
        if (!a) throw std::runtime_error("[AudioLevels] null amts file");
        if (al->t.channels != 2) throw std::runtime_error("[AudioLevels] the amts audio timeline is 16-bit stereo: the object must have 2 channels");
        batch_cover(al, first_frame, nframes);
        if (nframes == 0) return;
        if (!h_out) throw std::runtime_error("[AudioLevels] null output pointer");
        c->bind();
        for (int f = first_frame, end = first_frame + nframes; f < end;) {
            const int n = std::min(kAmtsChunkFrames, end - f);
            const Cover cv = batch_cover(al, f, n);
            const size_t elems = (size_t)(cv.hi - cv.lo) * 2, recs = (size_t)n * AMTGPU_AL_WORDS;
            if (elems) {
                if (al->host.size() < elems) al->host.resize(elems);
                amt_amts_read_audio(a, wavepath, cv.lo, cv.hi - cv.lo, al->host.data());
                if (al->dPcm.size() < elems) al->dPcm.alloc(elems);
                if (!amtgpu_frames_upload(c, al->dPcm.get(), al->host.data(), elems * sizeof(int16_t)) || !amtgpu_frames_upload_wait(c))
                    throw std::runtime_error(c->err);
            }
            if (al->dOut.size() < recs) al->dOut.alloc(recs);
            levels_batch(al, al->dPcm.get(), cv.lo, cv.hi - cv.lo, f, n, (uint64_t*)al->dOut.get());
            // (synchronises: the host buffer and the two device buffers are free for the next chunk)
            download_via_pinned(c, h_out + (size_t)(f - first_frame) * AMTGPU_AL_WORDS, al->dOut.get(), recs * sizeof(uint64_t));
            f += n;
        }
    });
}

int amtgpu_cm_mute_sections(const uint64_t* levels, int nframes, int mute_level, int min_frames, int* start_out, int* end_out, int cap, int* nmute)
{
    try {
        if (nframes < 0 || min_frames < 1 || (nframes > 0 && !levels)) return 0;
        const std::vector<std::pair<int, int>> ms = mute_sections(levels, nframes, mute_level, min_frames);
        if (nmute) *nmute = (int)ms.size();
        for (int i = 0; i < (int)ms.size() && i < cap; ++i) {
            if (start_out) start_out[i] = ms[(size_t)i].first;
            if (end_out) end_out[i] = ms[(size_t)i].second;
        }
        return (int)ms.size() <= cap ? 1 : 0;
    } catch (...) { return 0; }
}

// chapter_exe's output as CMAnalyze::readSceneChanges parses it (CMAnalyze.hpp:411-439) and as join_logo_scp gets it (:346-347): header,
// a "----" line, then "mute<k>: <a> - <b>" lines (regex mute\s*(\d+):\s*(\d+)\s*-\s*(\d+), tried first) and "SCPos: <frame>" lines.  A
// section's line stands in front of every scene change at or behind its start; a scene change belongs to a section when it lies in
// [start, end + 1] -- a cut on the first sounding frame is the section's.
int amtgpu_cm_write_chapter_exe_mute(const int* scene_changes, int nsc, const int* mute_start, const int* mute_end, int nmute, int nframes,
                                     int only_muted, const char* path)
{
    if (nsc < 0 || nmute < 0 || nframes < 0 || !path || (nsc > 0 && !scene_changes) || (nmute > 0 && (!mute_start || !mute_end))) return 0;
    for (int i = 1; i < nsc; ++i)
        if (scene_changes[i] < scene_changes[i - 1]) return 0;
    for (int j = 0; j < nmute; ++j)
        if (mute_start[j] < 0 || mute_start[j] > mute_end[j] || mute_end[j] >= nframes || (j > 0 && mute_start[j] <= mute_end[j - 1])) return 0;
    FILE* fp = std::fopen(path, "w");
    if (!fp) return 0;
    std::fprintf(fp, "amtgpu scene changes (self-specified field-difference detector) and silent sections (self-specified peak level), %d frames\n", nframes);
    std::fprintf(fp, "----------------------------------------\n");
    int j = 0;          // sections written so far
    auto sections_up_to = [&](long long frame) {
        for (; j < nmute && mute_start[j] <= frame; ++j) std::fprintf(fp, "mute%2d: %d - %d\n", j + 1, mute_start[j], mute_end[j]);
    };
    for (int i = 0; i < nsc; ++i) {
        const int sc = scene_changes[i];
        sections_up_to(sc);
        // (the sections written are those that start at or before sc, in ascending order and disjoint: only the last can still reach it)
        const bool member = j > 0 && sc <= (long long)mute_end[j - 1] + 1;
        if (only_muted && !member) continue;
        std::fprintf(fp, "\tSCPos: %d %d\n", sc, sc);
    }
    sections_up_to((long long)nframes);
    const bool ok = !std::ferror(fp);
    return std::fclose(fp) == 0 && ok ? 1 : 0;
}

} // extern "C"
