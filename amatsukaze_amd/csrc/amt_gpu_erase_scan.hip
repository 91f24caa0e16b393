// amt_gpu_erase_scan.hip -- C ABI part 2: AMTEraseLogo, LogoScan, ScanLogo.
#include "build_knobs.h"
#include "../../include/amt_gpu.h"

#include <cfloat>
#include <cmath>
#include <cstring>
#include <fstream>
#include <memory>
#include <numeric>
#include <sstream>

#include "api_common.hpp"
#include "logo_fit.hpp"

using namespace amt;

// ---------------------------------------------------------------------------------------------
// AMTEraseLogo
// ---------------------------------------------------------------------------------------------
struct AmtGpuErase {
    AmtGpuContext* ctx;
    LogoPlanes logo;
    std::vector<int> frameState;    // empty = no logoframe file (always analyse)
    bool haveLogof = false;
    std::string logofText;
    int mode = 0, maxFade = 16;
    bool zeroIdentity = false;      // every a*s + b*maxv of this logo is finite: Delogo with fade 0 returns the frame unchanged
    DevBuf<float> dPlanes;
    // the caller's fades go through two pinned slots (each with its own device copy and event), so that a batch returns without
    // waiting for the stream: a slot is rewritten only after the upload that read it has completed
    float2* hFades[2] = {nullptr, nullptr};
    size_t fadesCap[2] = {0, 0};
    DevBuf<float2> dFades[2];
    hipEvent_t fadesUploaded[2] = {nullptr, nullptr};
    int fadeSlot = 0;
    DevBuf<uint8_t> dState;         // frameState on the device (amtgpu_erase_calc_fades_device), for dStateFrames frames
    int dStateFrames = -1;
    ~AmtGpuErase()
    {
        for (int i = 0; i < 2; ++i) {
            if (hFades[i]) (void)hipHostFree(hFades[i]);
            if (fadesUploaded[i]) (void)hipEventDestroy(fadesUploaded[i]);
        }
    }
};

static AmtGpuErase* erase_new(AmtGpuContext* c, LogoPlanes logo, const std::string& logofText, bool haveLogof, int mode, int maxfade)
{
    std::unique_ptr<AmtGpuErase> er(new AmtGpuErase);
    er->ctx = c;
    er->logo = std::move(logo);
    er->mode = mode;
    er->maxFade = maxfade;
    er->haveLogof = haveLogof;
    er->logofText = logofText;
    if (haveLogof) (void)parse_logoframe(logofText, 0);     // report a malformed file at construction, like the filter does
    // fade 0: dst = (pixel)min(max(0*bg + 1*s + 0.5, 0), maxv) == s as long as bg = a*s + b*maxv cannot overflow to inf / NaN
    er->zeroIdentity = true;
    for (float v : er->logo.data) er->zeroIdentity = er->zeroIdentity && std::fabs(v) < 1e30f;
    c->bind();
    er->dPlanes.upload(er->logo.data, c->stream);
    return er.release();
}

extern "C" {

AmtGpuErase* amtgpu_erase_create(AmtGpuContext* c, const char* logopath, const char* logofpath, int mode, int maxfade)
{
    AmtGpuErase* er = nullptr;
    guard(c, [&] {
        LogoPlanes P;
        try { P = load_lgd(logopath); }
        catch (const std::exception&) { throw std::runtime_error(std::string("Failed to read logo file (") + logopath + ")"); }
        std::string text;
        const bool have = logofpath && logofpath[0];
        if (have) {
            std::ifstream f(logofpath, std::ios::binary);
            if (!f) throw std::runtime_error(std::string("Failed to read dat file (") + logofpath + ")");
            std::stringstream ss;
            ss << f.rdbuf();
            text = ss.str();
        }
        er = erase_new(c, std::move(P), text, have, mode, maxfade);
    });
    return er;
}

AmtGpuErase* amtgpu_erase_create_from_logo(AmtGpuContext* c, const AmtGpuLogo* logo, const char* logof_text, int mode, int maxfade)
{
    AmtGpuErase* er = nullptr;
    guard(c, [&] {
        const bool have = logof_text && logof_text[0];
        er = erase_new(c, logo->planes, have ? logof_text : "", have, mode, maxfade);
    });
    return er;
}

void amtgpu_erase_destroy(AmtGpuErase* er) { delete er; }

int amtgpu_erase_calc_fades(AmtGpuErase* er, const float* analysis, int num_frames, int first, int nframes, float* fades_out)
{
    return guard(er->ctx, [&] {
        if (first < 0 || nframes < 0 || first + nframes > num_frames) throw std::runtime_error("frame range outside the clip");
        if (er->haveLogof && (int)er->frameState.size() != num_frames) er->frameState = parse_logoframe(er->logofText, num_frames);
        static const std::vector<int> none;
        for (int i = 0; i < nframes; ++i) {
            const FadePair fp = fade_for_frame(er->haveLogof ? er->frameState : none, er->maxFade, analysis, num_frames, first + i);
            fades_out[2 * i] = fp.top;
            fades_out[2 * i + 1] = fp.bottom;
        }
    });
}

// what every Delogo entry checks before it looks at the planes; false: an empty batch, nothing to do
static bool erase_wanted(const AmtGpuErase* er, int bits, int nframes)
{
    if (bits < 8 || bits > 16) throw std::runtime_error("[AMTEraseLogo] Unsupported pixel format");
    if (er->mode != 0) throw std::runtime_error("[AMTEraseLogo] only mode 0 is supported (debug overlay modes are out of scope)");
    return nframes > 0;
}

// the batch's fades on the device: the caller's device array, or its host array through the pinned slots
static const float2* erase_fades(AmtGpuErase* er, int nframes, const float* fades, const float* d_fades)
{
    if (d_fades) return reinterpret_cast<const float2*>(d_fades);
    if (!fades) throw std::runtime_error("[AMTEraseLogo] null fades");
    const int slot = er->fadeSlot;
    er->fadeSlot ^= 1;
    if (!er->fadesUploaded[slot]) AMT_HIP(hipEventCreateWithFlags(&er->fadesUploaded[slot], hipEventDisableTiming));
    else AMT_HIP(hipEventSynchronize(er->fadesUploaded[slot]));          // the upload two batches ago
    if (er->fadesCap[slot] < (size_t)nframes) {
        if (er->hFades[slot]) AMT_HIP(hipHostFree(er->hFades[slot]));
        er->hFades[slot] = nullptr;
        AMT_HIP(hipHostMalloc((void**)&er->hFades[slot], (size_t)nframes * sizeof(float2), hipHostMallocDefault));
        er->fadesCap[slot] = (size_t)nframes;
        er->dFades[slot].alloc(nframes);                                   // hipFree waits for the kernels that read the old copy
    }
    std::memcpy(er->hFades[slot], fades, (size_t)nframes * sizeof(float2));
    AMT_HIP(hipMemcpyAsync(er->dFades[slot].get(), er->hFades[slot], (size_t)nframes * sizeof(float2), hipMemcpyHostToDevice, er->ctx->stream));
    AMT_HIP(hipEventRecord(er->fadesUploaded[slot], er->ctx->stream));
    return er->dFades[slot].get();
}

// Delogo of a batch that has passed erase_wanted: reads src, writes dst (laid out like src; the same planes for the in-place calls).
// rect_only: the planes hold the logo's rectangle and nothing else.  `span`: the profile span the call records, whichever kernel runs
static void erase_run(AmtGpuErase* er, const char* span, int bits, const FrameBatch& src, const PlanesOut& dst, bool rect_only, int nframes,
                      const float* fades, const float* d_fades)
{
    const LogoPlanes& P = er->logo;
    if (rect_only && (src.pitchY < P.w || src.pitchUV < P.wUV())) throw std::runtime_error("[AMTEraseLogo] rectangle pitch smaller than the logo width");
    er->ctx->bind();
    const float2* dfades = erase_fades(er, nframes, fades, d_fades);
    EraseGeom g;
    g.w = P.w; g.h = P.h; g.wUV = P.wUV(); g.hUV = P.hUV();
    // rectangle-only planes start at the logo's top-left sample; the chroma row parity is a property of the logo's position in
    // the frame (LogoScan.hpp:1374-1397), not of the buffer
    g.imgx = rect_only ? 0 : P.imgx; g.imgy = rect_only ? 0 : P.imgy;
    g.cx = rect_only ? 0 : P.imgx >> P.logUVx; g.cy = rect_only ? 0 : P.imgy >> P.logUVy;
    g.uvparity = (P.imgy / 2) % 2;
    const int sp = er->ctx->prof_begin(span);
    // fade 0 returns a sample unchanged only while the sample is <= maxv: min(tmp + 0.5, maxv) (LogoScan.hpp:1258) clamps the out-of-range
    // container values of a 9..15-bit LSB clip.  At 8 and 16 bits every container value is in range, and an MSB sample
    // (container >> (16 - bits)) can never exceed maxv: only there are fade-0 frames skipped.
    const bool skip_fade0 = er->zeroIdentity && (bits == 8 || bits == 16 || src.shift != 0);
    // planar LSB batches are delogo_kernel's, every other layout delogo_surfaces_kernel's
    if (!src.interleaved && !src.shift)
        AMT_HIP(launch_delogo(er->ctx->stream, bits, src, dst, er->dPlanes.get(), g, nframes, dfades, skip_fade0 ? 1 : 0));
    else
        AMT_HIP(launch_delogo_surfaces(er->ctx->stream, bits, src, dst, er->dPlanes.get(), g, nframes, dfades, skip_fade0 ? 1 : 0));
    er->ctx->prof_end(sp);
}

// the five entry points that take planes: in place when the source planes are the destination's
static void erase_planes(AmtGpuErase* er, const void* sY, const void* sU, const void* sV, void* dY, void* dU, void* dV, int64_t strideY, int64_t strideUV,
                         int pitchY, int pitchUV, int bits, int nframes, const float* fades, const float* d_fades, bool rect_only)
{
    if (!erase_wanted(er, bits, nframes)) return;
    const FrameBatch src = plane_batch(bits, sY, sU, sV, strideY, strideUV, pitchY, pitchUV);
    erase_run(er, "delogo_kernel", bits, src, PlanesOut{dY, dU, dV}, rect_only, nframes, fades, d_fades);
}

int amtgpu_erase_batch(AmtGpuErase* er, void* dY, void* dU, void* dV, int64_t strideY, int64_t strideUV, int pitchY,
                       int pitchUV, int bits, int nframes, const float* fades)
{
    return guard(er->ctx, [&] { erase_planes(er, dY, dU, dV, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, bits, nframes, fades, nullptr, false); });
}

int amtgpu_erase_rect_batch(AmtGpuErase* er, void* dY, void* dU, void* dV, int64_t strideY, int64_t strideUV, int pitchY,
                            int pitchUV, int bits, int nframes, const float* fades)
{
    return guard(er->ctx, [&] { erase_planes(er, dY, dU, dV, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, bits, nframes, fades, nullptr, true); });
}

int amtgpu_erase_batch_dfades(AmtGpuErase* er, void* dY, void* dU, void* dV, int64_t strideY, int64_t strideUV, int pitchY,
                              int pitchUV, int bits, int nframes, const float* d_fades)
{
    return guard(er->ctx, [&] {
        if (!d_fades && nframes > 0) throw std::runtime_error("[AMTEraseLogo] null device fades");
        erase_planes(er, dY, dU, dV, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, bits, nframes, nullptr, d_fades, false);
    });
}

int amtgpu_erase_rect_batch_dfades(AmtGpuErase* er, void* dY, void* dU, void* dV, int64_t strideY, int64_t strideUV, int pitchY,
                                   int pitchUV, int bits, int nframes, const float* d_fades)
{
    return guard(er->ctx, [&] {
        if (!d_fades && nframes > 0) throw std::runtime_error("[AMTEraseLogo] null device fades");
        erase_planes(er, dY, dU, dV, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, bits, nframes, nullptr, d_fades, true);
    });
}

int amtgpu_erase_batch_dfades_to(AmtGpuErase* er, const void* sY, const void* sU, const void* sV, void* dY, void* dU, void* dV, int64_t strideY,
                                 int64_t strideUV, int pitchY, int pitchUV, int bits, int nframes, const float* d_fades)
{
    return guard(er->ctx, [&] {
        if (!d_fades && nframes > 0) throw std::runtime_error("[AMTEraseLogo] null device fades");
        if (nframes > 0 && (!sY || !sU || !sV || !dY || !dU || !dV)) throw std::runtime_error("[AMTEraseLogo] null plane");
        erase_planes(er, sY, sU, sV, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, bits, nframes, nullptr, d_fades, false);
    });
}

// Delogo on decoder surfaces where they lie: src is read, dst (laid out like src; the same descriptor for the in-place calls) is written
static void erase_surfaces(AmtGpuErase* er, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes, const float* fades, const float* d_fades,
                           bool device_fades)
{
    const char* who = "[AMTEraseLogo]";
    auto refuse = [who](const char* what) { throw std::runtime_error(std::string(who) + " " + what); };
    if (nframes < 0) refuse("negative frame count");
    if (nframes == 0) return;
    const FrameBatch b = surface_batch(src, who);
    const int bits = src->bits;
    if (!erase_wanted(er, bits, nframes)) return;
    if (device_fades ? !d_fades : !fades) refuse(device_fades ? "null device fades" : "null fades");
    const LogoPlanes& P = er->logo;
    if (b.pitchY < P.imgx + P.w) refuse("surface pitchY smaller than the rectangle's rows");
    if (b.pitchUV < (b.interleaved ? 2 : 1) * ((P.imgx >> P.logUVx) + P.wUV())) refuse("surface pitchUV smaller than the rectangle's rows");
    PlanesOut out{const_cast<void*>(b.Y), const_cast<void*>(b.U), const_cast<void*>(b.V)};
    if (dst != src) {
        const FrameBatch d = surface_batch(dst, who);
        if (dst->bits != src->bits || d.interleaved != b.interleaved || d.shift != b.shift || d.pitchY != b.pitchY || d.pitchUV != b.pitchUV ||
            d.strideY != b.strideY || d.strideUV != b.strideUV)
            refuse("destination surfaces differ from the source's in bits, interleaved, msb_aligned, pitches or strides");
        out = PlanesOut{const_cast<void*>(d.Y), const_cast<void*>(d.U), const_cast<void*>(d.V)};
    }
    // (a planar LSB descriptor is an ordinary plane batch and records what the plane calls record)
    erase_run(er, !b.interleaved && !b.shift ? "delogo_kernel" : "delogo_surfaces_kernel", bits, b, out, false, nframes, fades, d_fades);
}

int amtgpu_erase_surfaces(AmtGpuErase* er, const AmtGpuSurfaces* batch, int nframes, const float* fades)
{
    return guard(er->ctx, [&] { erase_surfaces(er, batch, batch, nframes, fades, nullptr, false); });
}

int amtgpu_erase_surfaces_dfades(AmtGpuErase* er, const AmtGpuSurfaces* batch, int nframes, const float* d_fades)
{
    return guard(er->ctx, [&] { erase_surfaces(er, batch, batch, nframes, nullptr, d_fades, true); });
}

int amtgpu_erase_surfaces_dfades_to(AmtGpuErase* er, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes, const float* d_fades)
{
    return guard(er->ctx, [&] { erase_surfaces(er, src, dst, nframes, nullptr, d_fades, true); });
}

// CalcFade / CalcFade2 on the device (erase_scan_kernels.hip calc_fades_kernel); the host routine above stays the checker's
// counterpart and what the per-frame filter layer uses
int amtgpu_erase_calc_fades_device(AmtGpuErase* er, const float* d_analysis, int analysis_first, int analysis_count, int num_frames,
                                   int first, int nframes, float* d_fades_out)
{
    return guard(er->ctx, [&] {
        if (first < 0 || nframes < 0 || first + nframes > num_frames) throw std::runtime_error("frame range outside the clip");
        if (nframes == 0) return;
        if (!d_analysis || !d_fades_out) throw std::runtime_error("[AMTEraseLogo] null device pointer");
        // every record the decision of [first, first + nframes) can read: n - 8 .. n + 8, clamped the reference's way (which keeps
        // reads at the clip's ends inside the first / last eight frames)
        const int need0 = std::max(0, first - 8), need1 = std::min(num_frames, first + nframes + 8);
        if (analysis_first < 0 || analysis_count <= 0 || analysis_first > need0 || analysis_first + analysis_count < need1)
            throw std::runtime_error("[AMTEraseLogo] the analysis records do not cover frames first-8 .. first+nframes+8 (CalcFade2's window)");
        er->ctx->bind();
        const uint8_t* dstate = nullptr;
        if (er->haveLogof) {
            if ((int)er->frameState.size() != num_frames) er->frameState = parse_logoframe(er->logofText, num_frames);
            if (er->dStateFrames != num_frames) {
                std::vector<uint8_t> st(num_frames);
                for (int i = 0; i < num_frames; ++i) st[i] = (uint8_t)er->frameState[i];
                er->dState.upload(st, er->ctx->stream);          // (synchronous: once per clip)
                er->dStateFrames = num_frames;
            }
            dstate = er->dState.get();
        }
        const int sp = er->ctx->prof_begin("calc_fades_kernel");
        AMT_HIP(launch_calc_fades(er->ctx->stream, d_analysis, analysis_first, analysis_count, num_frames, first, nframes, dstate,
                                  er->maxFade >> 1, reinterpret_cast<float2*>(d_fades_out)));
        er->ctx->prof_end(sp);
    });
}

int amtgpu_erase_get_rect(const AmtGpuErase* er, int* out5)
{
    if (!er || !out5) return 0;
    const LogoPlanes& P = er->logo;
    out5[0] = P.imgx; out5[1] = P.imgy; out5[2] = P.w; out5[3] = P.h; out5[4] = er->zeroIdentity ? 1 : 0;
    return 1;
}

} // extern "C"

// ---------------------------------------------------------------------------------------------
// LogoScan
// ---------------------------------------------------------------------------------------------
struct AmtGpuLogoScan {
    AmtGpuContext* ctx;
    ScanSums sums;
    int thy = 0;
    DevBuf<unsigned long long> dAcc;
    DevBuf<int4> dVerdict, dAccepted;
    std::vector<int4> lastVerdicts;      // verdicts of the most recent add_batch (frame-local)
    std::vector<int4> accHost;           // accepted list of the most recent add_batch: source of an async upload, so it
    hipEvent_t accUploaded = nullptr;    //   lives here and is rewritten only after this event
    ~AmtGpuLogoScan() { if (accUploaded) (void)hipEventDestroy(accUploaded); }
    bool accDirty = false;               // device accumulators newer than sums.px
};

static void logoscan_pull(AmtGpuLogoScan* s)
{
    if (!s->accDirty) return;
    s->ctx->bind();
    download_via_pinned(s->ctx, s->sums.px.data(), s->dAcc.get(), s->sums.px.size() * sizeof(int64_t));
    s->accDirty = false;
}

// border verdicts for a batch (8..12 bits) of the scan's rectangle at r's origin, then accumulate the accepted subset; returns accepted count
static int logoscan_add(AmtGpuLogoScan* s, const FrameBatch& b, const ScanRect& r, int bits, int nframes, int max_valid, const uint8_t* use_mask,
                        uint8_t* valid_out, const int* frame_ids /* optional: batch slot -> frame index in b */,
                        const int4* known_verdicts /* optional: skip the border kernel */)
{
    ScanSums& S = s->sums;
    if (r.w != S.w || r.h != S.h) throw std::runtime_error("scan size mismatch");       // (the accumulators are sized for S)
    s->ctx->bind();
    std::vector<int4>& v = s->lastVerdicts;
    if (known_verdicts) {
        v.assign(known_verdicts, known_verdicts + nframes);
    } else {
        // the border histogram has 1 << bits bins and holds an accepted plane's samples, which span at most thy (erase_scan_kernels.hip
        // border_plane); 8-bit samples fit whatever thy is
        if (bits > 8 && s->thy >= (1 << bits)) throw std::runtime_error("[LogoScan] thy must be below 1 << bits for a clip of more than 8 bits");
        if (s->dVerdict.size() < (size_t)nframes) s->dVerdict.alloc(nframes);
        const int spb = s->ctx->prof_begin("scan_border_kernel");
        AMT_HIP(launch_scan_border(s->ctx->stream, bits, b, r, s->thy, nframes, s->dVerdict.get()));
        s->ctx->prof_end(spb);
        v.resize(nframes);
        download_via_pinned(s->ctx, v.data(), s->dVerdict.get(), (size_t)nframes * sizeof(int4));
    }
    std::vector<int4>& acc = s->accHost;
    if (s->accUploaded) AMT_HIP(hipEventSynchronize(s->accUploaded));
    else AMT_HIP(hipEventCreateWithFlags(&s->accUploaded, hipEventDisableTiming));
    acc.clear();
    for (int i = 0; i < nframes; ++i) {
        if (valid_out) valid_out[i] = 0;
        if ((int)acc.size() >= max_valid) continue;          // stream order: later frames are not even looked at
        if (use_mask && !use_mask[i]) continue;
        if (!v[i].x) continue;
        if (valid_out) valid_out[i] = 1;
        acc.push_back(make_int4(frame_ids ? frame_ids[i] : i, v[i].y, v[i].z, v[i].w));
        S.plane[0] += v[i].y; S.plane[1] += (int64_t)v[i].y * v[i].y;
        S.plane[2] += v[i].z; S.plane[3] += (int64_t)v[i].z * v[i].z;
        S.plane[4] += v[i].w; S.plane[5] += (int64_t)v[i].w * v[i].w;
    }
    if (!acc.empty()) {
        if (s->dAccepted.size() < acc.size()) s->dAccepted.alloc(acc.size());
        AMT_HIP(hipMemcpyAsync(s->dAccepted.get(), acc.data(), acc.size() * sizeof(int4), hipMemcpyHostToDevice, s->ctx->stream));
        AMT_HIP(hipEventRecord(s->accUploaded, s->ctx->stream));
        const int spa = s->ctx->prof_begin("scan_accumulate_kernel");
        AMT_HIP(launch_scan_accumulate(s->ctx->stream, bits, b, r, s->dAccepted.get(), (int)acc.size(), s->dAcc.get()));
        s->ctx->prof_end(spa);
        s->accDirty = true;
        S.nframes += (int)acc.size();
    }
    return (int)acc.size();
}

static AmtGpuLogoScan* logoscan_new(AmtGpuContext* c, int w, int h, int logUVx, int logUVy, int thy)
{
    if (w <= 0 || h <= 0 || (w & 1) || (h & 1) || logUVx != 1 || logUVy != 1)
        throw std::runtime_error("[LogoScan] rectangle must be even-sized 4:2:0");
    std::unique_ptr<AmtGpuLogoScan> s(new AmtGpuLogoScan);
    s->ctx = c;
    s->thy = thy;
    s->sums.w = w; s->sums.h = h; s->sums.logUVx = logUVx; s->sums.logUVy = logUVy;
    s->sums.px.assign(s->sums.npixels() * 3, 0);
    c->bind();
    s->dAcc.alloc(s->sums.px.size());
    AMT_HIP(hipMemsetAsync(s->dAcc.get(), 0, s->sums.px.size() * sizeof(int64_t), c->stream));
    AMT_HIP(hipStreamSynchronize(c->stream));
    return s.release();
}

extern "C" {

AmtGpuLogoScan* amtgpu_logoscan_create(AmtGpuContext* c, int w, int h, int logUVx, int logUVy, int thy)
{
    AmtGpuLogoScan* s = nullptr;
    guard(c, [&] { s = logoscan_new(c, w, h, logUVx, logUVy, thy); });
    return s;
}
void amtgpu_logoscan_destroy(AmtGpuLogoScan* s) { delete s; }

int amtgpu_logoscan_add_batch(AmtGpuLogoScan* s, const void* dY, const void* dU, const void* dV, int64_t strideY, int64_t strideUV,
                              int pitchY, int pitchUV, int bits, int imgx, int imgy, int nframes, int max_valid,
                              const uint8_t* use_mask, uint8_t* valid_out, int* naccepted)
{
    return guard(s->ctx, [&] {
        if (bits < 8 || bits > 12) throw std::runtime_error("[LogoScan] 8..12 bit only");
        const int n = logoscan_add(s, plane_batch(bits, dY, dU, dV, strideY, strideUV, pitchY, pitchUV), scan_rect(imgx, imgy, s->sums.w, s->sums.h),
                                   bits, nframes, max_valid, use_mask, valid_out, nullptr, nullptr);
        if (naccepted) *naccepted = n;
    });
}

int amtgpu_logoscan_nframes(const AmtGpuLogoScan* s) { return s->sums.nframes; }

int amtgpu_logoscan_get_sums(AmtGpuLogoScan* s, int64_t* sums, int64_t* plane_sums)
{
    return guard(s->ctx, [&] {
        logoscan_pull(s);
        if (sums) std::memcpy(sums, s->sums.px.data(), s->sums.px.size() * sizeof(int64_t));
        if (plane_sums) std::memcpy(plane_sums, s->sums.plane, sizeof s->sums.plane);
    });
}

int amtgpu_logoscan_set_sums(AmtGpuLogoScan* s, const int64_t* sums, const int64_t* plane_sums, int nframes)
{
    return guard(s->ctx, [&] {
        std::memcpy(s->sums.px.data(), sums, s->sums.px.size() * sizeof(int64_t));
        std::memcpy(s->sums.plane, plane_sums, sizeof s->sums.plane);
        s->sums.nframes = nframes;
        s->ctx->bind();
        AMT_HIP(hipMemcpyAsync(s->dAcc.get(), s->sums.px.data(), s->sums.px.size() * sizeof(int64_t), hipMemcpyHostToDevice, s->ctx->stream));
        AMT_HIP(hipStreamSynchronize(s->ctx->stream));
        s->accDirty = false;
    });
}

AmtGpuLogo* amtgpu_logoscan_get_logo(AmtGpuLogoScan* s, int maxv, int clean, int imgw, int imgh, int imgx, int imgy)
{
    AmtGpuLogo* l = nullptr;
    guard(s->ctx, [&] {
        logoscan_pull(s);
        std::unique_ptr<AmtGpuLogo> n(new AmtGpuLogo);
        if (!fit_logo(s->sums, maxv, clean != 0, n->planes)) throw std::runtime_error("Insufficient logo frames");
        n->planes.imgw = imgw; n->planes.imgh = imgh; n->planes.imgx = imgx; n->planes.imgy = imgy;
        l = n.release();
    });
    return l;
}

} // extern "C" (helpers)

namespace {

// The frames round 0 kept, which every later step reads again: where they lie and what their border said.
struct KeptFrames {
    FrameBatch planes{};              // the resident clip, or a session's store
    ScanRect r{};                     // the scan rectangle in those planes
    int bits = 8;
    std::vector<int> index;           // frame index in `planes` of every kept frame
    std::vector<int4> verdict;        // its {1, bgY, bgU, bgV}
    int count() const { return (int)index.size(); }
    // 3 * samples of the rectangle: the size of a scan's sums
    size_t npx() const { return (size_t)3 * ((size_t)r.w * r.h + 2 * (size_t)r.wUV * r.hUV); }
};
// what the finished logo's header says about the frame and the rectangle's place in it
struct LogoHeader { int imgw, imgh, imgx, imgy; };

// logoscan_add from known verdicts: the kept frames that `use` admits (all of them without one), no border kernel
using ::logoscan_add;
int logoscan_add(AmtGpuLogoScan* s, const KeptFrames& k, const uint8_t* use = nullptr)
{
    return k.count() ? logoscan_add(s, k.planes, k.r, k.bits, k.count(), k.count(), use, nullptr, k.index.data(), k.verdict.data()) : 0;
}

// sums of all ranks -> every rank (px sums, plane sums, frame count, and the ranks' status riding along); npx = 3 * samples of the
// scan rectangle (known even when this rank has no scan object to contribute)
void reduce_scan(AmtGpuLogoScan* s, ShardGuard& sg, size_t npx)
{
    if (!sg.sharded()) return;
    std::vector<int64_t> buf(npx + 8, 0);
    sg.attempt([&] {
        if (!s) throw std::runtime_error("no scan to reduce");
        logoscan_pull(s);
        if (s->sums.px.size() != npx) throw std::runtime_error("scan size mismatch");
        std::copy(s->sums.px.begin(), s->sums.px.end(), buf.begin());
        for (int k = 0; k < 6; ++k) buf[npx + k] = s->sums.plane[k];
        buf[npx + 6] = s->sums.nframes;
    });
    sg.allreduce(buf);
    if (!amtgpu_logoscan_set_sums(s, buf.data(), buf.data() + npx, (int)buf[npx + 6])) throw std::runtime_error(s->ctx->err);
}

// round 0's sums of a rank's share of the kept frames, summed over the ranks
void accumulate_kept(ShardGuard& sg, AmtGpuLogoScan* scan, const KeptFrames& kept)
{
    sg.attempt([&] { logoscan_add(scan, kept); });
    reduce_scan(scan, sg, kept.npx());
}

// ReMakeLogo twice (LogoScan.hpp:923-1036, 1065-1071) over the kept frames (maxv wherever the 8-bit text says 255, as AMTAnalyzeLogo
// does, :1130), starting from round 0's sums in scan0
std::unique_ptr<AmtGpuLogo> remake_rounds(AmtGpuContext* c, ShardGuard& sg, AmtGpuLogoScan* scan0, const KeptFrames& kept, const LogoHeader& hd, int thy)
{
    const ScanRect& r = kept.r;
    const int maxv = (1 << kept.bits) - 1;
    const int numFrames = kept.count();
    std::unique_ptr<AmtGpuLogo> logo(amtgpu_logoscan_get_logo(scan0, maxv, 0, hd.imgw, hd.imgh, hd.imgx, hd.imgy));
    if (!logo) throw std::runtime_error(c->err);
    DevBuf<int> dMap;
    if (numFrames) dMap.upload(kept.index, c->stream);
    std::vector<float> fades(20);
    for (int fi = 0; fi < 20; ++fi) fades[fi] = 0.1f * fi;
    DevBuf<float> dEval((size_t)std::max(1, numFrames) * 20);
    std::vector<float> hEval((size_t)numFrames * 20);
    for (int round = 0; round < 2; ++round) {
        std::unique_ptr<AmtGpuLogoScan> rescan;
        // (the regression that produced `logo` ran on the same reduced sums on every rank: all ranks are here, or none)
        sg.attempt([&] {
            EvalLogoSpec S;
            S.planes = deinterlaced_logo(logo->planes);
            S.tables = build_mask_tables(S.planes, 0.1f);
            S.imgx = r.imgx; S.imgy = r.imgy; S.row0 = 0; S.row_step = 1; S.deint = 1; S.out_off = 0;
            std::vector<EvalLogoSpec> specs;
            specs.push_back(std::move(S));
            EvalEngine eng(c, std::move(specs), fades, true, 20, "logo_eval_fused_kernel.remake");
            std::vector<uint8_t> use(numFrames, 0);
            if (numFrames) {
                eng.run(kept.planes, kept.bits, numFrames, dEval.get(), dMap.get());      // (reads the Y planes alone)
                download_via_pinned(c, hEval.data(), dEval.get(), hEval.size() * sizeof(float));
            }
            for (int i = 0; i < numFrames; ++i) {
                float best = FLT_MAX;
                int bestIdx = 0;
                for (int fi = 0; fi < 20; ++fi)
                    if (hEval[(size_t)i * 20 + fi] < best) { best = hEval[(size_t)i * 20 + fi]; bestIdx = fi; }
                use[i] = bestIdx > 8;                       // logo clearly present in this frame
            }
            sg.progress(50.0f + 25.0f * round + 12.5f, numFrames, numFrames, numFrames);
            rescan.reset(logoscan_new(c, r.w, r.h, 1, 1, thy));
            logoscan_add(rescan.get(), kept, use.data());
        });
        reduce_scan(rescan.get(), sg, kept.npx());
        logo.reset(amtgpu_logoscan_get_logo(rescan.get(), maxv, 1, hd.imgw, hd.imgh, hd.imgx, hd.imgy));
        if (!logo) throw std::runtime_error(c->err);
    }
    return logo;
}

// what every ScanLogo ends with, once round 0's sums of the kept frames are in `scan` on every rank: the two rounds, and rank 0 saves
void finish_logo(AmtGpuContext* c, ShardGuard& sg, AmtGpuLogoScan* scan, const KeptFrames& kept, const LogoHeader& hd, int thy, int serviceid,
                 const char* dstpath)
{
    const std::unique_ptr<AmtGpuLogo> logo = remake_rounds(c, sg, scan, kept, hd, thy);
    sg.progress(1, kept.count(), kept.count(), kept.count());
    if (dstpath && sg.writes()) save_lgd(logo->planes, dstpath, "No Name", serviceid);
}

} // namespace

// ---------------------------------------------------------------------------------------------
// ScanLogo as a session fed with frame batches: what InitialLogoCreator::onFrame does per decoded frame (LogoScan.hpp:881-914) -- border
// verdict, keep the rectangle of a valid frame until numMaxFrames are kept -- per batch, with the rectangles kept in HBM instead of the
// reference's lossless work file; the finish is MakeInitialLogo's regression and the two ReMakeLogo rounds over that store.
// ---------------------------------------------------------------------------------------------
struct AmtGpuScanLogoStream {
    AmtGpuContext* ctx = nullptr;
    int imgw = 0, imgh = 0, thy = 0, numMaxFrames = 0;
    int bits = 8, es = 1;                       // depth of the clip, bytes per sample
    ScanRect rect{};                            // the rectangle in a full frame
    std::unique_ptr<AmtGpuLogoScan> scan;       // the feeds' border verdicts; round 0's sums, accumulated from the store at the finish
    DevBuf<uint8_t> storeY, storeU, storeV;     // rectangles of the kept frames, tight: Y [n][h][w], U / V [n][h/2][w/2] samples of es bytes
    int cap = 0;                                // frames the store has room for
    std::vector<int4> keptVerdict;              // {1, bgY, bgU, bgV} of every kept frame
    int64_t nread = 0;                          // readCount (:883): frames consumed up to and including the one that closed the stream
    bool done = false, spent = false;
    // batch-local indices of a feed's kept frames: pinned, rewritten only after the upload that read it (keepUploaded)
    int* hKeep = nullptr;
    size_t keepCap = 0;
    DevBuf<int> dKeep;
    hipEvent_t keepUploaded = nullptr;
    // feed_surfaces: the rectangle of a batch of decoder surfaces as planar LSB planes, tight like the store; grows to the largest batch seen
    DevBuf<uint8_t> surfY, surfU, surfV;
    int surfCap = 0;
    int nkept() const { return (int)keptVerdict.size(); }
    size_t slotY() const { return (size_t)rect.w * rect.h * es; }           // bytes of one kept frame's luma / chroma rectangle
    size_t slotC() const { return (size_t)rect.wUV * rect.hUV * es; }
    ~AmtGpuScanLogoStream()
    {
        if (keepUploaded) { (void)hipEventSynchronize(keepUploaded); (void)hipEventDestroy(keepUploaded); }
        if (hKeep) (void)hipHostFree(hKeep);
    }
};

namespace {

AmtGpuScanLogoStream* stream_new(AmtGpuContext* c, int imgw, int imgh, int bits, int imgx, int imgy, int w, int h, int thy, int numMaxFrames)
{
    const int es = scan_sample_bytes(bits, thy);
    if (imgx < 0 || imgy < 0 || w > imgw - imgx || h > imgh - imgy) throw std::runtime_error("scan rectangle outside the frame");
    std::unique_ptr<AmtGpuScanLogoStream> s(new AmtGpuScanLogoStream);
    s->ctx = c;
    s->imgw = imgw; s->imgh = imgh; s->thy = thy;
    s->bits = bits; s->es = es;
    s->numMaxFrames = std::max(0, numMaxFrames);
    s->scan.reset(logoscan_new(c, w, h, 1, 1, thy));       // (refuses odd and non-positive sizes)
    s->rect = scan_rect(imgx, imgy, w, h);
    s->done = s->numMaxFrames == 0;
    // the store grows with what is kept: numMaxFrames is a limit (callers pass 1 << 30), not a size
    s->cap = std::max(1, std::min(s->numMaxFrames, 256));
    s->storeY.alloc(s->cap * s->slotY());
    s->storeU.alloc(s->cap * s->slotC());
    s->storeV.alloc(s->cap * s->slotC());
    AMT_HIP(hipEventCreateWithFlags(&s->keepUploaded, hipEventDisableTiming));
    return s.release();
}

// room for `need` kept frames: the store doubles, what it holds moves on the stream
void stream_reserve(AmtGpuScanLogoStream* s, int need)
{
    if (need <= s->cap) return;
    const int ncap = (int)std::min<int64_t>(s->numMaxFrames, std::max<int64_t>(need, 2 * (int64_t)s->cap));
    const size_t ysz = s->slotY(), csz = s->slotC(), n = (size_t)s->nkept();
    DevBuf<uint8_t> nY(ysz * ncap), nU(csz * ncap), nV(csz * ncap);
    if (n) {
        hipStream_t st = s->ctx->stream;
        AMT_HIP(hipMemcpyAsync(nY.get(), s->storeY.get(), ysz * n, hipMemcpyDeviceToDevice, st));
        AMT_HIP(hipMemcpyAsync(nU.get(), s->storeU.get(), csz * n, hipMemcpyDeviceToDevice, st));
        AMT_HIP(hipMemcpyAsync(nV.get(), s->storeV.get(), csz * n, hipMemcpyDeviceToDevice, st));
        AMT_HIP(hipStreamSynchronize(st));                   // the old store is freed below
    }
    s->storeY = std::move(nY); s->storeU = std::move(nU); s->storeV = std::move(nV);
    s->cap = ncap;
}

// the next nframes frames of the stream; rect_only: the planes hold the rectangle alone
void stream_feed(AmtGpuScanLogoStream* s, const void* dY, const void* dU, const void* dV, int64_t strideY, int64_t strideUV, int pitchY, int pitchUV,
                 int nframes, bool rect_only)
{
    if (s->spent) throw std::runtime_error("[ScanLogo] the session has been finished");
    if (nframes < 0) throw std::runtime_error("[ScanLogo] negative frame count");
    if (nframes == 0 || s->done) return;
    if (!dY || !dU || !dV) throw std::runtime_error("[ScanLogo] null plane");
    const ScanRect r = rect_only ? scan_rect(0, 0, s->rect.w, s->rect.h) : s->rect;
    if (pitchY < r.imgx + r.w || pitchUV < r.cx + r.wUV) throw std::runtime_error("[ScanLogo] pitch smaller than the rectangle's rows");
    const FrameBatch b = plane_batch(s->bits, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, PlaneRules::ScanLogo);
    AmtGpuContext* c = s->ctx;
    // verdicts alone (quota 0): which valid frames count is decided here, in stream order
    logoscan_add(s->scan.get(), b, r, s->bits, nframes, 0, nullptr, nullptr, nullptr, nullptr);
    const std::vector<int4>& v = s->scan->lastVerdicts;
    AMT_HIP(hipEventSynchronize(s->keepUploaded));
    if (s->keepCap < (size_t)nframes) {
        if (s->hKeep) AMT_HIP(hipHostFree(s->hKeep));
        s->hKeep = nullptr; s->keepCap = 0;
        AMT_HIP(hipHostMalloc((void**)&s->hKeep, (size_t)nframes * sizeof(int), hipHostMallocDefault));
        s->keepCap = (size_t)nframes;
        s->dKeep.alloc(nframes);
    }
    const int first = s->nkept(), room = s->numMaxFrames - first;      // room > 0: the stream is open
    int m = 0, consumed = nframes;
    for (int i = 0; i < nframes; ++i) {
        if (!v[i].x) continue;
        s->hKeep[m++] = i;
        if (m == room) { consumed = i + 1; break; }
    }
    if (m) {
        stream_reserve(s, first + m);
        AMT_HIP(hipMemcpyAsync(s->dKeep.get(), s->hKeep, (size_t)m * sizeof(int), hipMemcpyHostToDevice, c->stream));
        AMT_HIP(hipEventRecord(s->keepUploaded, c->stream));
        const int sp = c->prof_begin("scan_keep_kernel");
        AMT_HIP(launch_scan_keep(c->stream, b, r, s->dKeep.get(), m, PlanesOut{s->storeY.get(), s->storeU.get(), s->storeV.get()}, first));
        c->prof_end(sp);
        for (int k = 0; k < m; ++k) s->keptVerdict.push_back(v[s->hKeep[k]]);
    }
    s->nread += consumed;
    s->done = m == room;
}

// the next nframes frames of the stream as decoder surfaces: their rectangle through the session's scratch, then stream_feed's rect_only path
void stream_feed_surfaces(AmtGpuScanLogoStream* s, const AmtGpuSurfaces* batch, int nframes)
{
    if (s->spent) throw std::runtime_error("[ScanLogo] the session has been finished");
    if (nframes < 0) throw std::runtime_error("[ScanLogo] negative frame count");
    if (nframes == 0 || s->done) return;
    if (!batch) throw std::runtime_error("[ScanLogo] null surface descriptor");
    if (batch->bits != s->bits) throw std::runtime_error("[ScanLogo] surfaces of another depth than the session's");
    const ScanRect& r = s->rect;
    if (!batch->interleaved && !batch->msb_aligned) {
        // planar LSB planes are what feed takes
        stream_feed(s, batch->Y, batch->U, batch->V, batch->strideY, batch->strideUV, batch->pitchY, batch->pitchUV, nframes, false);
        return;
    }
    AmtGpuContext* c = s->ctx;
    (void)surface_batch(batch, "[ScanLogo]");              // a bad descriptor is refused before the scratch is touched
    if (s->surfCap < nframes) {
        // (hipFree waits for the kernels that still read the old scratch)
        s->surfCap = 0;
        s->surfY.alloc(s->slotY() * nframes);
        s->surfU.alloc(s->slotC() * nframes);
        s->surfV.alloc(s->slotC() * nframes);
        s->surfCap = nframes;
    }
    surfaces_extract(c, batch, "[ScanLogo]", r, nframes, PlanesOut{s->surfY.get(), s->surfU.get(), s->surfV.get()}, (int64_t)s->slotY(), (int64_t)s->slotC(),
                     r.w, r.wUV);
    stream_feed(s, s->surfY.get(), s->surfU.get(), s->surfV.get(), (int64_t)s->slotY(), (int64_t)s->slotC(), r.w, r.wUV, nframes, true);
}

// MakeInitialLogo's regression and the two ReMakeLogo rounds over the store (LogoScan.hpp:845-848, 1065-1071); sharded: this rank's share of
// the quota first, as the resident driver hands it out
void stream_finish(AmtGpuScanLogoStream* s, const AmtGpuCollectives* coll, int serviceid, const char* dstpath, AMTGPU_LOGO_ANALYZE_CB cb)
{
    const bool usable = !coll || coll->world <= 1 || (coll->allgather && coll->allreduce_sum_i64 && coll->rank >= 0 && coll->rank < coll->world);
    ShardGuard sg(usable ? coll : nullptr, cb);
    // (a spent session on one rank of a sharded finish must not strand the others: its refusal rides along like any other failure)
    sg.attempt([&] { if (s->spent) throw std::runtime_error("[ScanLogo] the session has been finished"); });
    s->spent = true;
    if (!usable) throw std::runtime_error("AmtGpuCollectives incomplete");
    if (!sg.sharded() && !dstpath) throw std::runtime_error("[ScanLogo] null destination path");
    s->ctx->bind();
    const int n = sg.quota_share(s->nkept(), s->numMaxFrames);
    const ScanRect r = scan_rect(0, 0, s->rect.w, s->rect.h);
    // (the store is tight: a slot's bytes apart)
    const FrameBatch store = plane_batch(s->bits, s->storeY.get(), s->storeU.get(), s->storeV.get(), (int64_t)s->slotY(), (int64_t)s->slotC(), r.w, r.wUV);
    KeptFrames kept{store, r, s->bits, std::vector<int>(n), std::vector<int4>(s->keptVerdict.begin(), s->keptVerdict.begin() + n)};
    std::iota(kept.index.begin(), kept.index.end(), 0);          // the store holds the kept frames alone, in order
    accumulate_kept(sg, s->scan.get(), kept);
    finish_logo(s->ctx, sg, s->scan.get(), kept, LogoHeader{s->imgw, s->imgh, s->rect.imgx, s->rect.imgy}, s->thy, serviceid, dstpath);
}

void stream_report(const AmtGpuScanLogoStream* s, int64_t* nread, int* nkept, int* done)
{
    if (nread) *nread = s->nread;
    if (nkept) *nkept = s->nkept();
    if (done) *done = s->done ? 1 : 0;
}

} // namespace

extern "C" {

AmtGpuScanLogoStream* amtgpu_scanlogo_stream_create_bits(AmtGpuContext* c, int imgw, int imgh, int bits, int imgx, int imgy, int w, int h, int thy,
                                                         int numMaxFrames)
{
    if (!c) return nullptr;
    AmtGpuScanLogoStream* s = nullptr;
    guard(c, [&] { s = stream_new(c, imgw, imgh, bits, imgx, imgy, w, h, thy, numMaxFrames); });
    return s;
}

AmtGpuScanLogoStream* amtgpu_scanlogo_stream_create(AmtGpuContext* c, int imgw, int imgh, int imgx, int imgy, int w, int h, int thy,
                                                    int numMaxFrames)
{
    return amtgpu_scanlogo_stream_create_bits(c, imgw, imgh, 8, imgx, imgy, w, h, thy, numMaxFrames);
}

void amtgpu_scanlogo_stream_destroy(AmtGpuScanLogoStream* s) { delete s; }

int amtgpu_scanlogo_stream_feed(AmtGpuScanLogoStream* s, const void* dY, const void* dU, const void* dV, int64_t strideY, int64_t strideUV,
                                int pitchY, int pitchUV, int nframes, int* nkept, int* done)
{
    if (!s) return 0;
    return guard(s->ctx, [&] {
        stream_feed(s, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, nframes, false);
        stream_report(s, nullptr, nkept, done);
    });
}

int amtgpu_scanlogo_stream_feed_rect(AmtGpuScanLogoStream* s, const void* dY, const void* dU, const void* dV, int64_t strideY, int64_t strideUV,
                                     int pitchY, int pitchUV, int nframes, int* nkept, int* done)
{
    if (!s) return 0;
    return guard(s->ctx, [&] {
        stream_feed(s, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, nframes, true);
        stream_report(s, nullptr, nkept, done);
    });
}

int amtgpu_scanlogo_stream_feed_surfaces(AmtGpuScanLogoStream* s, const AmtGpuSurfaces* batch, int nframes, int* nkept, int* done)
{
    if (!s) return 0;
    return guard(s->ctx, [&] {
        stream_feed_surfaces(s, batch, nframes);
        stream_report(s, nullptr, nkept, done);
    });
}

int amtgpu_scanlogo_stream_status(const AmtGpuScanLogoStream* s, int64_t* nread, int* nkept, int* done)
{
    if (!s) return 0;
    return guard(s->ctx, [&] { stream_report(s, nread, nkept, done); });
}

int amtgpu_scanlogo_stream_finish(AmtGpuScanLogoStream* s, int serviceid, const char* dstpath, AMTGPU_LOGO_ANALYZE_CB cb)
{
    if (!s) return 0;
    return guard(s->ctx, [&] { stream_finish(s, nullptr, serviceid, dstpath, cb); });
}

int amtgpu_scanlogo_stream_finish_sharded(AmtGpuScanLogoStream* s, const AmtGpuCollectives* coll, int serviceid, const char* dstpath,
                                          AMTGPU_LOGO_ANALYZE_CB cb)
{
    if (!s) return 0;
    return guard(s->ctx, [&] { stream_finish(s, coll, serviceid, dstpath, cb); });
}

int amtgpu_scanlogo_bits(AmtGpuContext* c, const void* dY, const void* dU, const void* dV, int64_t strideY, int64_t strideUV,
                         int pitchY, int pitchUV, int imgw, int imgh, int bits, int nframes, int serviceid, const char* dstpath, int imgx,
                         int imgy, int w, int h, int thy, int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb)
{
    return amtgpu_scanlogo_sharded_bits(c, nullptr, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, imgw, imgh, bits, nframes, serviceid, dstpath, imgx,
                                        imgy, w, h, thy, numMaxFrames, cb);
}

int amtgpu_scanlogo(AmtGpuContext* c, const void* dY, const void* dU, const void* dV, int64_t strideY, int64_t strideUV,
                    int pitchY, int pitchUV, int imgw, int imgh, int nframes, int serviceid, const char* dstpath, int imgx,
                    int imgy, int w, int h, int thy, int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb)
{
    return amtgpu_scanlogo_bits(c, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, imgw, imgh, 8, nframes, serviceid, dstpath, imgx, imgy, w, h,
                                thy, numMaxFrames, cb);
}

// The reference's exported ScanLogo, argument for argument (LogoScan.hpp:1083-1098; C# P/Invoke AmatsukazeNatives.cs:391-393), over a
// raw 4:2:0 clip file instead of a transport stream (decode is out of scope): int32 {'AMTR', width, height, nframes} followed by
// tight 8-bit Y, U, V planes per frame, or int32 {'AMTH', width, height, nframes, bits} (bits 9..12) followed by the same planes as
// little-endian uint16 (amt_read_raw_clip_header, api_common.hpp).  Frames are streamed through the pinned ring in chunks and fed to a
// ScanLogo session (above): only the rectangles of accepted frames stay in HBM for the two ReMakeLogo rounds (the reference keeps them
// in `workfile` through a lossless codec, :840-912 -- here the argument is accepted and the file left untouched).
int amtgpu_scanlogo_file(AmtGpuContext* c, const char* srcpath, int serviceid, const char* workfile, const char* dstpath, int imgx, int imgy,
                         int w, int h, int thy, int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb)
{
    (void)workfile;
    return guard(c, [&] {
        ShardGuard one(nullptr, cb);
        RawClipReader in(c, srcpath, false);
        const int W = in.hd.width, N = in.hd.frames;
        std::unique_ptr<AmtGpuScanLogoStream> s(stream_new(c, W, in.hd.height, in.hd.bits, imgx, imgy, w, h, thy, numMaxFrames));
        while (!s->done && in.next()) {
            stream_feed(s.get(), in.dY, in.dU, in.dV, (int64_t)in.ysz, (int64_t)in.csz, W, W / 2, in.n, false);      // (strides in bytes, pitches in samples)
            one.progress(50.0f * in.nread / std::max(1, N), in.nread, 0, s->nkept());
        }
        stream_finish(s.get(), nullptr, serviceid, dstpath, cb);
    });
}

int amtgpu_scanlogo_fileW(AmtGpuContext* c, const uint16_t* srcpath, int serviceid, const uint16_t* workfile, const uint16_t* dstpath, int imgx,
                          int imgy, int w, int h, int thy, int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb)
{
    const std::string src = amt_utf8_from_utf16z(srcpath), work = amt_utf8_from_utf16z(workfile), dst = amt_utf8_from_utf16z(dstpath);
    return amtgpu_scanlogo_file(c, src.c_str(), serviceid, work.c_str(), dst.c_str(), imgx, imgy, w, h, thy, numMaxFrames, cb);
}

// LogoAnalyzer::ScanLogo (LogoScan.hpp:1058-1079): initial logo from every flat-bordered frame (stop at
// numMaxFrames), then twice: evaluate 20 fades per kept frame, re-accumulate only frames whose best fade
// index is > 8, regress again with clean-up; save.
//
// coll != nullptr: this rank holds one contiguous shard of the stream.  What is global in the reference's three
// sequential rounds is (a) which valid frames fall inside the numMaxFrames quota ("first N in stream order", :885) and
// (b) the accumulators each regression reads -- both integers, so an all-gather of valid counts and an all-reduce of
// int64 sums reproduce the single-GPU result exactly; the regression then runs redundantly on every rank.
//
// Every resident entry point ends here; coll == nullptr or world 1: the whole stream, one rank.
int amtgpu_scanlogo_sharded_bits(AmtGpuContext* c, const AmtGpuCollectives* coll, const void* dY, const void* dU, const void* dV,
                                 int64_t strideY, int64_t strideUV, int pitchY, int pitchUV, int imgw, int imgh, int bits, int nframes_local,
                                 int serviceid, const char* dstpath, int imgx, int imgy, int w, int h, int thy, int numMaxFrames,
                                 AMTGPU_LOGO_ANALYZE_CB cb)
{
    if (!c) return 0;
    return guard(c, [&] {
        (void)scan_sample_bytes(bits, thy);                  // (refused before anything is exchanged: the same on every rank)
        ShardGuard sg(coll, cb);
        if (sg.sharded() && (!coll->allgather || !coll->allreduce_sum_i64 || coll->rank < 0 || coll->rank >= coll->world))
            throw std::runtime_error("AmtGpuCollectives incomplete");
        KeptFrames kept;                    // (indices within this rank's frames)
        kept.r = scan_rect(imgx, imgy, w, h);
        kept.bits = bits;
        const ScanRect& r = kept.r;
        std::unique_ptr<AmtGpuLogoScan> scan;
        const int chunk = 4096;
        // round 0: the border verdicts of every frame in stream order.  One rank accepts frames as it goes and stops once numMaxFrames are
        // kept; a shard accepts nothing yet (quota 0) and keeps every valid frame: which of them count is decided below
        auto wanted = [&] { return sg.sharded() || kept.count() < numMaxFrames; };
        sg.attempt([&] {
            if (r.imgx < 0 || r.imgy < 0 || r.imgx + r.w > imgw || r.imgy + r.h > imgh) throw std::runtime_error("scan rectangle outside the frame");
            kept.planes = plane_batch(bits, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, PlaneRules::ScanLogo);
            scan.reset(logoscan_new(c, r.w, r.h, 1, 1, thy));
            for (int f0 = 0; f0 < nframes_local && wanted(); f0 += chunk) {
                const int n = std::min(chunk, nframes_local - f0);
                logoscan_add(scan.get(), plane_batch_from(kept.planes, f0), r, bits, n, sg.sharded() ? 0 : numMaxFrames - kept.count(), nullptr,
                             nullptr, nullptr, nullptr);
                for (int i = 0; i < n; ++i)
                    if (scan->lastVerdicts[i].x && wanted()) { kept.index.push_back(f0 + i); kept.verdict.push_back(scan->lastVerdicts[i]); }
                sg.progress(50.0f * (f0 + n) / std::max(1, nframes_local), f0 + n, 0, kept.count());
            }
        });
        if (sg.sharded()) {
            // this rank's share of the quota (and how every rank is doing), accumulated locally, summed over ranks
            const int quota = sg.quota_share(kept.count(), numMaxFrames);
            kept.index.resize(quota);
            kept.verdict.resize(quota);
            accumulate_kept(sg, scan.get(), kept);
        }
        finish_logo(c, sg, scan.get(), kept, LogoHeader{imgw, imgh, r.imgx, r.imgy}, thy, serviceid, dstpath);
    });
}

int amtgpu_scanlogo_sharded(AmtGpuContext* c, const AmtGpuCollectives* coll, const void* dY, const void* dU, const void* dV,
                            int64_t strideY, int64_t strideUV, int pitchY, int pitchUV, int imgw, int imgh, int nframes_local,
                            int serviceid, const char* dstpath, int imgx, int imgy, int w, int h, int thy, int numMaxFrames,
                            AMTGPU_LOGO_ANALYZE_CB cb)
{
    return amtgpu_scanlogo_sharded_bits(c, coll, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, imgw, imgh, 8, nframes_local, serviceid, dstpath,
                                        imgx, imgy, w, h, thy, numMaxFrames, cb);
}

} // extern "C"
