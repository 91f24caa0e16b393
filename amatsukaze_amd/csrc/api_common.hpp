// api_common.hpp -- shared by the amt_gpu*.hip translation units that implement the C ABI.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <exception>
#include <fstream>
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

// Bytes per sample of a clip `bits` deep: bytes up to 8 bits, 16-bit little-endian containers above.
inline int sample_bytes(int bits) { return bits <= 8 ? 1 : 2; }

// The depths ScanLogo takes (8: bytes; 9..12: the range LogoColor::Add's int products hold) and thy against the border histogram, which
// has 1 << bits bins; returns the bytes per sample.  Refused before a plane is touched or anything is exchanged.
inline int scan_sample_bytes(int bits, int thy = 0)
{
    if (bits < 8 || bits > 12) throw std::runtime_error("[ScanLogo] bits must be 8..12");
    if (bits > 8 && thy >= (1 << bits)) throw std::runtime_error("[ScanLogo] thy must be below 1 << bits for a clip of more than 8 bits");
    return sample_bytes(bits);
}

// The ABI's description of a batch of planes (byte strides, sample pitches) as the launchers take it: the same units, planar and LSB.
// Nothing is converted here or anywhere else in the host code; this is the one place that checks that the sample size divides the byte
// strides, so that a launcher whose kernel counts in samples may divide (frame_batch.h, FrameBatch).  ScanLogo's entry points also refuse
// the depth and a plane base off the sample size, in their own words; a caller that reads the luma plane alone passes null chroma planes
// and a zero chroma stride.
enum class PlaneRules { Plain, ScanLogo };
inline amt::FrameBatch plane_batch(int bits, const void* Y, const void* U, const void* V, int64_t strideY, int64_t strideUV, int pitchY, int pitchUV,
                                   PlaneRules rules = PlaneRules::Plain)
{
    const bool scan = rules == PlaneRules::ScanLogo;
    const int es = scan ? scan_sample_bytes(bits) : sample_bytes(bits);
    if (strideY % es || strideUV % es)
        throw std::runtime_error(scan ? "[ScanLogo] odd byte stride for 16-bit samples" : "frame stride not a multiple of the sample size");
    if (scan && ((uintptr_t)Y % es || (uintptr_t)U % es || (uintptr_t)V % es)) throw std::runtime_error("[ScanLogo] plane base not aligned to the sample size");
    return amt::FrameBatch{Y, U, V, strideY, strideUV, pitchY, pitchUV, es, 0, 0};
}
// The luma batch of the plane entry points of the frame metrics and the logo finder (amtgpu_framestats_batch, _sharded, _logofind_add_batch,
// the raw-clip reader's chunks), and of nobody else.  It checks nothing: their kernels count the stride in bytes, so these calls have never
// refused a stride that the sample size does not divide, and must not start to.  A launcher that divides the stride needs plane_batch.
inline amt::FrameBatch luma_batch_unchecked(int bits, const void* Y, int64_t strideY, int pitchY)
{
    return amt::FrameBatch{Y, nullptr, nullptr, strideY, 0, pitchY, 0, sample_bytes(bits), 0, 0};
}

// A batch of decoder surfaces as the kernels take it, or a refusal in the caller's words (`who`: "[ScanLogo]", ...): the one place that
// reads an AmtGpuSurfaces.  luma_only: the chroma fields are not looked at (the logo finder).
inline amt::FrameBatch surface_batch(const AmtGpuSurfaces* s, const char* who, bool luma_only = false)
{
    auto refuse = [who](const char* what) { throw std::runtime_error(std::string(who) + " " + what); };
    if (!s) refuse("null surface descriptor");
    if (s->bits < 8 || s->bits > 16) refuse("surface bits must be 8..16");
    if (s->msb_aligned && s->bits == 8) refuse("MSB-aligned surfaces are 16-bit containers: bits must be 9..16");
    if (s->reserved != 0) refuse("reserved field of the surface descriptor must be 0");
    const int es = sample_bytes(s->bits);
    if (!s->Y || (!luma_only && (!s->U || (!s->interleaved && !s->V)))) refuse("null surface plane");
    if (s->strideY % es || (!luma_only && s->strideUV % es)) refuse("odd byte stride for 16-bit containers");
    if ((uintptr_t)s->Y % es || (!luma_only && ((uintptr_t)s->U % es || (!s->interleaved && (uintptr_t)s->V % es))))
        refuse("surface plane base not aligned to the container size");
    amt::FrameBatch b{s->Y, luma_only ? nullptr : s->U, luma_only || s->interleaved ? nullptr : s->V, s->strideY, luma_only ? 0 : s->strideUV,
                      s->pitchY, luma_only ? 0 : s->pitchUV, es, s->interleaved ? 1 : 0, s->msb_aligned ? 16 - s->bits : 0};
    return b;
}

// The rectangle r of nframes surfaces as planar LSB planes (dst strides in bytes, pitches in samples), enqueued on the context's stream:
// what amtgpu_surfaces_extract_rect does once its arguments are read, and what the ScanLogo session's feed_surfaces runs into its scratch.
inline void surfaces_extract(AmtGpuContext* c, const AmtGpuSurfaces* src, const char* who, const amt::ScanRect& r, int nframes, const amt::PlanesOut& dst,
                             int64_t dstrideY, int64_t dstrideUV, int dpitchY, int dpitchUV)
{
    auto refuse = [who](const char* what) { throw std::runtime_error(std::string(who) + " " + what); };
    if (nframes < 0) refuse("negative frame count");
    if (nframes == 0) return;
    const amt::FrameBatch b = surface_batch(src, who);
    if (r.imgx < 0 || r.imgy < 0 || r.w <= 0 || r.h <= 0 || (r.w & 1) || (r.h & 1)) refuse("rectangle must be even-sized and inside the surface");
    if (b.pitchY < r.imgx + r.w) refuse("surface pitchY smaller than the rectangle's rows");
    if (b.pitchUV < (b.interleaved ? 2 : 1) * (r.cx + r.wUV)) refuse("surface pitchUV smaller than the rectangle's rows");
    if (!dst.Y || !dst.U || !dst.V) refuse("null destination plane");
    if (dpitchY < r.w || dpitchUV < r.wUV) refuse("destination pitch smaller than the rectangle's rows");
    if (dstrideY % b.es || dstrideUV % b.es || (uintptr_t)dst.Y % b.es || (uintptr_t)dst.U % b.es || (uintptr_t)dst.V % b.es)
        refuse("destination not aligned to the sample size");
    c->bind();
    const int sp = c->prof_begin("surfaces_extract_kernel");
    AMT_HIP(amt::launch_surfaces_extract(c->stream, b, r, nframes, dst, dstrideY, dstrideUV, dpitchY, dpitchUV));
    c->prof_end(sp);
}

// The Y planes of a batch of surfaces (b: surface_batch's, luma_only) as the evaluation engines take a luma batch (EvalEngine::run,
// analyze_run): LSB samples, planar, no chroma.  The engines read rows [row0, row1) and columns [col0, col1) of every picture and
// nothing else.  LSB surfaces are passed as they lie.  MSB-aligned ones: that band of every picture -- from col0 rounded down to 64
// containers -- is copied as LSB samples (surfaces_extract_kernel with an empty chroma part) into `scratch`, which grows to the largest
// batch seen, rows a multiple of 64 samples apart, and the batch's base is where sample (0, 0) of picture 0 would lie in that layout:
// the engines' alignment-dependent choices are those of an aligned planar clip.  The scratch is the caller's (one per object: its
// surfaces entry points are not re-entrant).
inline amt::FrameBatch surfaces_luma_view(AmtGpuContext* c, const amt::FrameBatch& b, int row0, int row1, int col0, int col1, int nframes,
                                          amt::DevBuf<uint8_t>& scratch)
{
    if (!b.shift) return b;
    const int c0 = col0 & ~63, bw = col1 - c0, rows = row1 - row0;
    const int pitch = (bw + 63) & ~63;
    const size_t frame_bytes = (size_t)rows * pitch * b.es;
    // (a tail: the engines' aligned 8- and 16-byte accesses may end a few samples behind col1; where the band fills its pitch that is the
    // next row, and behind the last row of the last picture it must still be the allocation.  The front needs none: c0 is aligned down)
    const size_t need = frame_bytes * (size_t)nframes + 64;
    c->bind();
    if (scratch.size() < need) scratch.alloc(need);        // (hipFree waits for the kernels that still read the old scratch)
    uint8_t* band = scratch.get();
    const int sp = c->prof_begin("surfaces_extract_kernel");
    AMT_HIP(amt::launch_surfaces_extract(c->stream, b, amt::ScanRect{c0, row0, 0, 0, bw, rows, 0, 0}, nframes, amt::PlanesOut{band, nullptr, nullptr},
                                         (long long)frame_bytes, 0, pitch, 0));
    c->prof_end(sp);
    return amt::FrameBatch{band - ((size_t)row0 * pitch + c0) * b.es, nullptr, nullptr, (long long)frame_bytes, 0, pitch, 0, b.es, 0, 0};
}

// amtgpu_amts_read_audio (amts_file.cpp) for callers inside the library: throws instead of leaving a message on the file's context
void amt_amts_read_audio(const AmtGpuAmtsFile* a, const char* wavepath, int64_t start, int64_t count, int16_t* out);

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

// A sharded run must never leave ranks behind in a collective: a rank whose own work threw (a HIP error, a bad argument, a
// cancelled callback) keeps entering every exchange with neutral data, its status rides along, and ALL ranks throw right after
// the exchange in which the status becomes known.  One rank alone (coll null or world 1): plain exceptions.
struct ShardGuard {
    const AmtGpuCollectives* coll;               // nullptr: not sharded
    AMTGPU_LOGO_ANALYZE_CB cb;
    const char* what;                            // what the ranks abandon together, for the message
    std::string error;                           // this rank's failure, if any
    int64_t cancel = 0;
    ShardGuard(const AmtGpuCollectives* c, AMTGPU_LOGO_ANALYZE_CB cb_, const char* what_ = "run") : coll(c && c->world > 1 ? c : nullptr), cb(cb_), what(what_) {}
    bool sharded() const { return coll != nullptr; }
    bool writes() const { return !coll || coll->rank == 0; }       // rank 0 saves the result
    template <typename F> void attempt(F&& fn)
    {
        if (!sharded()) { fn(); return; }
        if (!error.empty()) return;
        try { fn(); } catch (const std::exception& e) { error = e.what(); } catch (...) { error = "unknown error"; }
    }
    void progress(float p, int nread, int total, int ngather)
    {
        if (!cb || cb(p, nread, total, ngather)) return;
        if (!sharded()) throw std::runtime_error("Cancel requested");
        cancel = 1;                              // the other ranks learn about it with the next exchange
    }
    int64_t status() const { return (cancel ? 1 : 0) + (error.empty() ? 0 : (int64_t)1 << 32); }
    // `summed` = sum over ranks of status(): everyone leaves together
    void agree(int64_t summed) const
    {
        if (!error.empty()) throw std::runtime_error(error);
        if (summed >> 32) throw std::runtime_error(std::string("another rank failed; the sharded ") + what + " was abandoned on every rank");
        if (summed & 0xFFFFFFFF) throw std::runtime_error("Cancel requested");
    }
    // buf summed over the ranks in place; its last element is the guard's: the status word (a failed rank contributes zeros)
    void allreduce(std::vector<int64_t>& buf) const
    {
        if (!error.empty()) std::fill(buf.begin(), buf.end(), 0);
        buf.back() = status();
        if (!coll->allreduce_sum_i64(coll->user, buf.data(), (int64_t)buf.size())) throw std::runtime_error("allreduce_sum_i64 failed");
        agree(buf.back());
    }
    // This rank's share of "the first numMaxFrames valid frames of the stream" (LogoScan.hpp:885; rank 0 holds the first frames), of which
    // it found nvalid: {count, status} of every rank is gathered, and the ranks before this one are served first.
    int quota_share(int nvalid, int numMaxFrames) const
    {
        if (!sharded()) return nvalid;
        std::vector<int64_t> counts((size_t)coll->world * 2, 0);
        const int64_t mine[2] = {error.empty() ? nvalid : 0, status()};
        if (!coll->allgather(coll->user, mine, counts.data(), sizeof mine)) throw std::runtime_error("allgather failed");
        int64_t before = 0, summed = 0;
        for (int k = 0; k < coll->world; ++k) summed += counts[2 * k + 1];
        for (int k = 0; k < coll->rank; ++k) before += counts[2 * k];
        agree(summed);
        return (int)std::max<int64_t>(0, std::min<int64_t>(mine[0], (int64_t)numMaxFrames - before));
    }
};

// A raw clip file (RawClipHeader above), read in chunks of min(1024, 256 MiB / frame bytes) frames: next() de-interleaves a chunk (file
// order is Y, U, V per frame; the device batch is plane-major, Y[n] U[n] V[n], or Y[n] alone with luma_only) and uploads it through the
// pinned ring.  The one device buffer is refilled by every chunk: next() first waits for the stream, on which the caller's work on the
// previous chunk runs.
struct RawClipReader {
    AmtGpuContext* ctx;
    std::ifstream file;
    RawClipHeader hd{};
    bool luma_only;
    size_t ysz = 0, csz = 0, fsz = 0;            // bytes of a frame's luma plane, of one chroma plane, of the frame: the batch's byte strides
    int chunk = 1, n = 0, nread = 0;             // frames per chunk, in the current one, handed out so far
    amt::DevBuf<uint8_t> dChunk;
    std::vector<uint8_t> host, planar;
    const uint8_t *dY = nullptr, *dU = nullptr, *dV = nullptr;       // the current chunk (dU, dV null with luma_only)
    RawClipReader(AmtGpuContext* c, const char* srcpath, bool luma_only_) : ctx(c), luma_only(luma_only_)
    {
        if (!srcpath) throw std::runtime_error("null source path");
        file.open(srcpath, std::ios::binary);
        if (!file) throw std::runtime_error(std::string("failed to open file ") + srcpath);
        hd = amt_read_raw_clip_header(file);
        const int es = sample_bytes(hd.bits);
        ysz = (size_t)hd.width * hd.height * es; csz = (size_t)(hd.width / 2) * (hd.height / 2) * es; fsz = ysz + 2 * csz;
        chunk = (int)std::max<size_t>(1, std::min<size_t>(1024, (256u << 20) / fsz));
        c->bind();
        dChunk.alloc((luma_only ? ysz : fsz) * chunk);
        host.resize(fsz * chunk);
        planar.resize((luma_only ? ysz : fsz) * chunk);
    }
    // the next chunk's planes on the device; false: the clip has been read
    bool next()
    {
        if (n) AMT_HIP(hipStreamSynchronize(ctx->stream));          // the chunk buffer is refilled by the upload below
        if (nread >= hd.frames) return false;
        n = std::min(chunk, hd.frames - nread);
        file.read(reinterpret_cast<char*>(host.data()), (std::streamsize)(fsz * n));
        if (!file) throw std::runtime_error("raw clip truncated");
        for (int i = 0; i < n; ++i) {
            std::memcpy(planar.data() + ysz * i, host.data() + fsz * i, ysz);
            if (luma_only) continue;
            std::memcpy(planar.data() + ysz * n + csz * i, host.data() + fsz * i + ysz, csz);
            std::memcpy(planar.data() + ysz * n + csz * n + csz * i, host.data() + fsz * i + ysz + csz, csz);
        }
        if (!amtgpu_frames_upload(ctx, dChunk.get(), planar.data(), (luma_only ? ysz : fsz) * n) || !amtgpu_frames_upload_wait(ctx)) throw std::runtime_error(ctx->err);
        dY = dChunk.get();
        dU = luma_only ? nullptr : dY + ysz * n;
        dV = luma_only ? nullptr : dU + csz * n;
        nread += n;
        return true;
    }
};
