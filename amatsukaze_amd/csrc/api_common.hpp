// api_common.hpp -- shared by the amt_gpu*.hip translation units that implement the C ABI.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <exception>
#include <istream>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/amt_gpu.h"
#include "decisions.hpp"
#include "engine.hpp"
#include "logo_model.hpp"

struct AmtGpuLogo {
    amt::LogoPlanes planes;
};

// UTF-16 (a Windows wchar_t string, NUL-terminated: what the reference's exports take, LogoScan.hpp:1083-1086) -> UTF-8.  A lone
// surrogate becomes U+FFFD: the result is always valid UTF-8.
inline std::string amt_utf8_from_utf16(const uint16_t* s, size_t n)
{
    std::string o;
    auto put = [&](uint32_t c) {
        if (c < 0x80) o += (char)c;
        else if (c < 0x800) { o += (char)(0xC0 | (c >> 6)); o += (char)(0x80 | (c & 0x3F)); }
        else if (c < 0x10000) { o += (char)(0xE0 | (c >> 12)); o += (char)(0x80 | ((c >> 6) & 0x3F)); o += (char)(0x80 | (c & 0x3F)); }
        else { o += (char)(0xF0 | (c >> 18)); o += (char)(0x80 | ((c >> 12) & 0x3F)); o += (char)(0x80 | ((c >> 6) & 0x3F)); o += (char)(0x80 | (c & 0x3F)); }
    };
    for (size_t i = 0; i < n; ++i) {
        uint32_t c = s[i];
        if (c >= 0xD800 && c < 0xDC00 && i + 1 < n && s[i + 1] >= 0xDC00 && s[i + 1] < 0xE000) {
            c = 0x10000 + ((c - 0xD800) << 10) + (s[i + 1] - 0xDC00);
            ++i;
        } else if (c >= 0xD800 && c < 0xE000) {
            c = 0xFFFD;
        }
        put(c);
    }
    return o;
}
inline std::string amt_utf8_from_utf16z(const uint16_t* s)
{
    if (!s) return std::string();
    size_t n = 0;
    while (s[n]) ++n;
    return amt_utf8_from_utf16(s, n);
}

// The header of a raw 4:2:0 clip file (amtgpu_scanlogo_file, _file_auto): little-endian int32 {'AMTR', width, height, frames} before tight
// 8-bit Y, U, V planes per frame, or {'AMTH', width, height, frames, bits} with bits 9..12 before the same planes as little-endian uint16.
struct RawClipHeader { int width, height, frames, bits; };
inline RawClipHeader amt_read_raw_clip_header(std::istream& f)
{
    int32_t hdr[5] = {0, 0, 0, 0, 8};
    f.read(reinterpret_cast<char*>(hdr), 4 * sizeof(int32_t));
    const bool hibit = f && hdr[0] == 0x48544D41;
    if (hibit) f.read(reinterpret_cast<char*>(hdr + 4), sizeof(int32_t));
    if (!f || (hdr[0] != 0x52544D41 && !hibit) || hdr[1] <= 0 || hdr[2] <= 0 || hdr[3] < 0 || (hdr[1] & 1) || (hdr[2] & 1))
        throw std::runtime_error("not a raw clip (int32 'AMTR', width, height, frames; 8-bit 4:2:0 planes -- or 'AMTH', width, height, frames, bits; "
                                 "16-bit containers)");
    if (hibit && (hdr[4] < 9 || hdr[4] > 12)) throw std::runtime_error("raw AMTH clip: bits must be 9..12 (8-bit clips are 'AMTR' files)");
    return RawClipHeader{hdr[1], hdr[2], hdr[3], hdr[4]};
}

// run f(); on any exception keep the message on the context and return 0 (no exceptions cross the ABI)
template <typename F> inline int guard(AmtGpuContext* c, F&& f, const char* caller = __builtin_FUNCTION())
{
    AMT_TRACE_SCOPE(caller);
    (void)caller;
    // calls on one context are serialised: its stream, staging ring, error string and timing spans are shared state
    std::unique_lock<std::recursive_mutex> lk;
    if (c) lk = std::unique_lock<std::recursive_mutex>(c->mu);
    try {
        f();
        return 1;
    } catch (const std::exception& e) {
        if (c) c->err = e.what();
    } catch (...) {
        if (c) c->err = "unknown error";
    }
    return 0;
}

// The exchange of per-frame records between the ranks of a sharded run (world > 1, coll->allgather present): this rank holds records
// [first, first + nlocal) of num_frames, rec_bytes each, at `local`; afterwards every rank's are in place in `out` (the whole clip's).
// Ragged shards: {first, nlocal, ok} is gathered first, then the records padded to the largest shard.  A rank whose own part failed
// (local_error) still enters every collective -- the others would block in it for ever -- and all ranks throw together once the status
// is known.  tiling: the ranges must tile the clip in rank order; otherwise any range inside the clip is taken.  false: no records.
inline bool allgather_records(const AmtGpuCollectives* coll, const void* local, int first, int nlocal, int64_t num_frames, size_t rec_bytes,
                              void* out, bool tiling, const std::string& local_error, const char* what)
{
    const bool ok = local_error.empty();
    const int64_t mine[3] = {ok ? first : 0, ok ? nlocal : 0, ok ? 1 : 0};
    std::vector<int64_t> ranges((size_t)coll->world * 3);
    if (!coll->allgather(coll->user, mine, ranges.data(), sizeof mine)) throw std::runtime_error("allgather failed");
    bool all_ok = true, inside = true, tiles = true;
    int64_t nmax = 0, next = 0;
    for (int r = 0; r < coll->world; ++r) {
        const int64_t f = ranges[3 * r], n = ranges[3 * r + 1];
        all_ok = all_ok && ranges[3 * r + 2] == 1;
        inside = inside && f >= 0 && n >= 0 && f + n <= num_frames;
        tiles = tiles && f == next && n >= 0;
        next = f + n;
        nmax = std::max(nmax, n);
    }
    tiles = tiles && next == num_frames;
    if (!ok) throw std::runtime_error(local_error);
    if (!all_ok) throw std::runtime_error(std::string("another rank failed before the exchange of ") + what);
    if (tiling && !tiles) throw std::runtime_error("the ranks' frame ranges do not tile the clip in rank order");
    if (!tiling && !inside) throw std::runtime_error("a rank reported a frame range outside the clip");
    if (nmax == 0 || rec_bytes == 0) return false;
    const size_t shard = (size_t)nmax * rec_bytes;
    std::vector<uint8_t> send(shard, 0), recv(shard * coll->world);
    if (nlocal) std::memcpy(send.data(), local, (size_t)nlocal * rec_bytes);
    if (!coll->allgather(coll->user, send.data(), recv.data(), (int64_t)shard)) throw std::runtime_error("allgather failed");
    for (int r = 0; r < coll->world; ++r) {
        const int64_t f = ranges[3 * r], n = ranges[3 * r + 1];
        if (n) std::memcpy((uint8_t*)out + (size_t)f * rec_bytes, recv.data() + (size_t)r * shard, (size_t)n * rec_bytes);
    }
    return true;
}
