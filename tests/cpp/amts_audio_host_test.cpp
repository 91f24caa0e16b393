// Stand-alone memory check of the amts audio reader (amatsukaze_amd/csrc/amts_file.cpp), meant for a sanitizer build on the host:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I<rocm>/include
//       amatsukaze_amd/csrc/amts_file.cpp tests/cpp/amts_audio_host_test.cpp -o amts_audio_host_test && ./amts_audio_host_test <dir>
// (amts_file.cpp needs ROCm's headers for the context type it shares with the rest of the library, and none of its runtime: nothing of
// libamdhip64 is linked.)  It writes an amts file and its wave file into <dir> -- a first audio frame without a wave, one more in the
// middle, a frame whose waveLength is short of what GetAudio reads, runs of frames in shuffled file order with odd gaps -- and drives
// amtgpu_amts_read_audio over reads that start mid-frame, span frames, run past the end and are empty, each into a heap buffer of exactly
// count * 4 bytes, against a per-frame restatement of AMTSource::GetAudio (AMTSource.hpp:782-817).  Exit status 0: all equal.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/amt_gpu.h"

namespace {

struct AudioFrame { int32_t frameIndex; int64_t waveOffset; int32_t waveLength; };

template <typename T> void put(std::vector<uint8_t>& b, T v)
{
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
    b.insert(b.end(), p, p + sizeof(T));
}

uint32_t rng_state = 12345;
uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

void write_file(const std::string& path, const std::vector<uint8_t>& b)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(b.data(), 1, b.size(), f) != b.size()) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
}

// SaveAMTSource's layout (AMTSource.hpp:835-852; amts_file.cpp's header comment): two UTF-16 strings, VideoFormat 44, AudioFormat 8,
// FilterSourceFrame[] (none), FilterAudioFrame[] 24 each, DecoderSetting 12
void write_amts(const std::string& path, const std::string& wavpath, const std::vector<AudioFrame>& frames)
{
    std::vector<uint8_t> b;
    for (const std::string& s : {std::string("src.ts"), wavpath}) {
        put<int64_t>(b, (int64_t)s.size());
        for (char c : s) put<uint16_t>(b, (uint16_t)(unsigned char)c);
    }
    b.resize(b.size() + 44, 0);
    put<int32_t>(b, 2); put<int32_t>(b, 48000);
    put<int64_t>(b, 0);
    put<int64_t>(b, (int64_t)frames.size());
    for (const AudioFrame& f : frames) {
        put<int32_t>(b, f.frameIndex); put<int32_t>(b, 0); put<int64_t>(b, f.waveOffset); put<int32_t>(b, f.waveLength); put<int32_t>(b, 0);
    }
    b.resize(b.size() + 12, 0);
    write_file(path, b);
}

// GetAudio, one audio frame at a time
std::vector<uint8_t> get_audio(const std::vector<uint8_t>& wave, const std::vector<AudioFrame>& frames, int64_t spf, int64_t start, int64_t count)
{
    std::vector<uint8_t> out((size_t)count * 4, 0xEE);
    uint8_t* ptr = out.data();
    for (int64_t k = start / spf, off = start % spf; count > 0 && k < (int64_t)frames.size(); ++k, off = 0) {
        const int64_t n = std::min<int64_t>(spf * 4 - off * 4, count * 4);
        if (frames[(size_t)k].waveLength != 0) std::memcpy(ptr, wave.data() + frames[(size_t)k].waveOffset + off * 4, (size_t)n);
        else std::memset(ptr, 0, (size_t)n);
        ptr += n;
        count -= n / 4;
    }
    if (count > 0) std::memset(ptr, 0, (size_t)count * 4);
    return out;
}

int failures = 0;
void expect(bool ok, const char* what, int64_t a = 0, int64_t b = 0)
{
    if (ok) return;
    std::fprintf(stderr, "FAILED: %s (%lld, %lld)\n", what, (long long)a, (long long)b);
    ++failures;
}

} // namespace

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    const std::string wavpath = dir + "/amts_audio_host_test.wav", amtspath = dir + "/amts_audio_host_test.dat";
    const int naudio = 23, spf = 96;
    const int zero_a = 0, zero_b = 11, short_frame = 4;

    // runs of 1..4 frames, the second half of the runs first in the file, 1..29 bytes of junk between them
    std::vector<std::vector<int>> runs;
    for (int k = 0; k < naudio;) {
        const int n = 1 + (int)(rnd() % 4);
        runs.emplace_back();
        for (int i = k; i < std::min(naudio, k + n); ++i) runs.back().push_back(i);
        k += n;
    }
    std::vector<std::vector<int>> order(runs.begin() + (long)runs.size() / 2, runs.end());
    order.insert(order.end(), runs.begin(), runs.begin() + (long)runs.size() / 2);
    std::vector<uint8_t> wave(44, 0x52);
    std::vector<AudioFrame> frames((size_t)naudio);
    for (const std::vector<int>& run : order) {
        for (uint32_t g = 1 + rnd() % 29; g; --g) wave.push_back((uint8_t)rnd());
        for (int f : run) {
            if (f == zero_a || f == zero_b) { frames[(size_t)f] = {f, 987654321, 0}; continue; }       // an offset far outside the file
            frames[(size_t)f] = {f, (int64_t)wave.size(), spf * 4 - (f == short_frame ? 8 : 0)};
            for (int i = 0; i < spf * 4; ++i) wave.push_back((uint8_t)rnd());
        }
    }
    // (no padding behind the last frame of the file: a read of one byte too many is a short read)
    write_file(wavpath, wave);
    write_amts(amtspath, wavpath, frames);

    AmtGpuAmtsFile* a = amtgpu_amts_load(nullptr, amtspath.c_str());
    if (!a) { std::fprintf(stderr, "amtgpu_amts_load failed\n"); return 2; }
    int got_spf = 0;
    int64_t ns = 0;
    expect(amtgpu_amts_audio_info(a, &got_spf, &ns) == 1 && got_spf == spf && ns == (int64_t)spf * naudio, "audio_info", got_spf, ns);
    std::vector<int> fi((size_t)naudio), wl((size_t)naudio);
    std::vector<int64_t> wo((size_t)naudio);
    expect(amtgpu_amts_get_audio_frames(a, fi.data(), wo.data(), wl.data()) == 1, "get_audio_frames");
    expect(amtgpu_amts_get_audio_frames(a, nullptr, nullptr, nullptr) == 1, "get_audio_frames with null columns");
    for (int k = 0; k < naudio; ++k)
        expect(fi[(size_t)k] == frames[(size_t)k].frameIndex && wo[(size_t)k] == frames[(size_t)k].waveOffset && wl[(size_t)k] == frames[(size_t)k].waveLength, "column", k);

    // every start in the first frames and around the zero-length ones, against a spread of counts; then a random sweep
    std::vector<std::pair<int64_t, int64_t>> reads;
    for (int64_t start : {0, 1, spf / 2, spf - 1, spf, spf + 1, zero_b * spf - 1, zero_b * spf, (zero_b + 1) * spf - 1, (int)ns - 1, (int)ns, (int)ns + 500})
        for (int64_t count : {0, 1, 2, spf - 1, spf, spf + 1, 3 * spf + 5, (int)ns, (int)ns + 77}) reads.emplace_back(start, count);
    for (int i = 0; i < 2000; ++i) reads.emplace_back((int64_t)(rnd() % (uint32_t)(ns + 50)), (int64_t)(rnd() % (uint32_t)(5 * spf)));
    for (const auto& r : reads) {
        const std::vector<uint8_t> want = get_audio(wave, frames, spf, r.first, r.second);
        // exactly count * 4 bytes on the heap: the sanitizer sees a write past either end
        int16_t* out = r.second ? static_cast<int16_t*>(std::malloc((size_t)r.second * 4)) : nullptr;
        if (out) std::memset(out, 0xEE, (size_t)r.second * 4);
        for (const char* path : {(const char*)nullptr, wavpath.c_str()}) {
            expect(amtgpu_amts_read_audio(a, path, r.first, r.second, out) == 1, "read_audio returned 0", r.first, r.second);
            expect(r.second == 0 || std::memcmp(out, want.data(), want.size()) == 0, "read_audio differs from GetAudio", r.first, r.second);
        }
        std::free(out);
    }

    // refusals
    int16_t four[8];
    expect(amtgpu_amts_read_audio(a, nullptr, -1, 2, four) == 0, "negative start taken");
    expect(amtgpu_amts_read_audio(a, nullptr, 0, -1, four) == 0, "negative count taken");
    expect(amtgpu_amts_read_audio(a, (dir + "/absent.wav").c_str(), spf, 2, four) == 0, "absent wave file taken");
    expect(amtgpu_amts_read_audio(nullptr, nullptr, 0, 2, four) == 0, "null file taken");
    std::vector<uint8_t> cut(wave.begin(), wave.end() - 1);                       // one byte short: the frame that lies last in the file
    write_file(dir + "/amts_audio_host_test_cut.wav", cut);
    std::vector<int16_t> whole((size_t)ns * 2);
    expect(amtgpu_amts_read_audio(a, (dir + "/amts_audio_host_test_cut.wav").c_str(), 0, ns, whole.data()) == 0, "short read taken");
    expect(amtgpu_amts_read_audio(a, wavpath.c_str(), 0, ns, whole.data()) == 1, "whole read refused");
    amtgpu_amts_destroy(a);

    write_amts(amtspath, wavpath, {});
    a = amtgpu_amts_load(nullptr, amtspath.c_str());
    if (!a) { std::fprintf(stderr, "amtgpu_amts_load failed\n"); return 2; }
    expect(amtgpu_amts_audio_info(a, &got_spf, &ns) == 1 && got_spf == 0 && ns == 0, "audio_info of a clip without audio");
    expect(amtgpu_amts_read_audio(a, wavpath.c_str(), 0, 2, four) == 0, "clip without audio taken");
    amtgpu_amts_destroy(a);

    std::printf(failures ? "amts_audio_host_test: %d FAILED\n" : "amts_audio_host_test: ok\n", failures);
    return failures ? 1 : 0;
}
