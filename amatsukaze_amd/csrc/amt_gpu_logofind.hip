// amt_gpu_logofind.hip -- C ABI of the automatic logo finder: the edge-persistence sums on the device (logofind_kernels.hip), their
// exchange between ranks, and ScanLogo fed with the best candidate (logo_find.cpp ranks them).  Self-specified: DESIGN.md section 6b.
#include "build_knobs.h"
#include "../../include/amt_gpu.h"

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "api_common.hpp"

using namespace amt;

struct AmtGpuLogoFind {
    AmtGpuContext* ctx;
    int width, height, bits;
    int num_cus;
    int64_t nframes = 0;
    DevBuf<unsigned long long> dSums;      // S1 [H][W] then SM [H][W]
};

namespace {

size_t npx(const AmtGpuLogoFind* lf) { return (size_t)lf->width * lf->height; }

AmtGpuLogoFind* logofind_new(AmtGpuContext* c, int width, int height, int bits)
{
    if (width < 3 || height < 3 || bits < 8 || bits > 16) throw std::runtime_error("[LogoFind] unsupported frame format (W, H >= 3, bits 8..16)");
    c->bind();
    std::unique_ptr<AmtGpuLogoFind> lf(new AmtGpuLogoFind{c, width, height, bits, 0});
    int dev = 0;
    AMT_HIP(hipGetDevice(&dev));
    AMT_HIP(hipDeviceGetAttribute(&lf->num_cus, hipDeviceAttributeMultiprocessorCount, dev));
    lf->dSums.alloc(2 * npx(lf.get()));
    AMT_HIP(hipMemsetAsync(lf->dSums.get(), 0, 2 * npx(lf.get()) * sizeof(unsigned long long), c->stream));
    return lf.release();
}

// b: the luma batch (b.shift > 0: MSB-aligned 16-bit containers, summed as container >> shift = 16 - bits)
void logofind_add(AmtGpuLogoFind* lf, const FrameBatch& b, int nframes)
{
    if (nframes < 0) throw std::runtime_error("[LogoFind] negative frame count");
    if (nframes == 0) return;
    if (!b.Y) throw std::runtime_error("[LogoFind] null frame pointer");
    if (b.pitchY < lf->width || b.strideY < 0) throw std::runtime_error("[LogoFind] pitch below the width or negative frame stride");
    lf->ctx->bind();
    const long long cap = logofind_launch_cap(lf->bits);
    const int sp = lf->ctx->prof_begin("logofind_kernel");
    for (long long f0 = 0; f0 < nframes; f0 += cap) {
        const int n = (int)std::min<long long>(cap, nframes - f0);
        AMT_HIP(launch_logofind(lf->ctx->stream, lf->bits, plane_batch_from(b, f0), lf->width, lf->height, n, lf->num_cus, lf->dSums.get(),
                                lf->dSums.get() + npx(lf)));
    }
    lf->ctx->prof_end(sp);
    lf->nframes += nframes;
}

std::vector<int64_t> logofind_pull(AmtGpuLogoFind* lf)
{
    std::vector<int64_t> h(2 * npx(lf));
    lf->ctx->bind();
    download_via_pinned(lf->ctx, h.data(), lf->dSums.get(), h.size() * sizeof(int64_t));
    return h;
}

void logofind_push(AmtGpuLogoFind* lf, const int64_t* sums, int64_t nframes)
{
    lf->ctx->bind();
    lf->dSums.upload((const unsigned long long*)sums, 2 * npx(lf), lf->ctx->stream);
    lf->nframes = nframes;
}

// the best candidate of the current sums, or throws "no logo found"
AmtGpuLogoRect best_rect(AmtGpuLogoFind* lf, const AmtGpuLogoFindParams* params)
{
    const std::vector<int64_t> h = logofind_pull(lf);
    AmtGpuLogoRect r{};
    int n = 0;
    if (!amtgpu_logofind_candidates_host(h.data(), lf->width, lf->height, lf->bits, lf->nframes, params, &r, 1, &n))
        throw std::runtime_error("[LogoFind] invalid detection parameters");
    if (n == 0) throw std::runtime_error("no logo found");
    return r;
}

// the sums of all ranks on every rank; a rank that failed before the exchange still enters it (its status rides along) so that nobody blocks
void logofind_reduce(AmtGpuLogoFind* lf, ShardGuard& sg)
{
    if (!sg.sharded()) return;
    if (!sg.coll->allreduce_sum_i64 || sg.coll->rank < 0 || sg.coll->rank >= sg.coll->world) throw std::runtime_error("AmtGpuCollectives incomplete");
    const size_t n = 2 * npx(lf);
    std::vector<int64_t> buf(n + 2, 0);
    sg.attempt([&] {
        const std::vector<int64_t> h = logofind_pull(lf);
        std::copy(h.begin(), h.end(), buf.begin());
        buf[n] = lf->nframes;
    });
    sg.allreduce(buf);
    logofind_push(lf, buf.data(), buf[n]);
}

void zero_found(AmtGpuLogoRect* found) { if (found) std::memset(found, 0, sizeof *found); }

} // namespace

extern "C" {

AmtGpuLogoFind* amtgpu_logofind_create(AmtGpuContext* c, int width, int height, int bits)
{
    AmtGpuLogoFind* lf = nullptr;
    if (!c) return nullptr;
    guard(c, [&] { lf = logofind_new(c, width, height, bits); });
    return lf;
}

void amtgpu_logofind_destroy(AmtGpuLogoFind* lf) { delete lf; }

int amtgpu_logofind_add_batch(AmtGpuLogoFind* lf, const void* dY, int64_t frame_stride, int pitch, int nframes)
{
    if (!lf) return 0;
    return guard(lf->ctx, [&] { logofind_add(lf, luma_batch_unchecked(lf->bits, dY, frame_stride, pitch), nframes); });
}

int amtgpu_logofind_add_surfaces(AmtGpuLogoFind* lf, const AmtGpuSurfaces* batch, int nframes)
{
    if (!lf) return 0;
    return guard(lf->ctx, [&] {
        if (nframes < 0) throw std::runtime_error("[LogoFind] negative frame count");
        if (nframes == 0) return;
        const FrameBatch b = surface_batch(batch, "[LogoFind]", true);
        if (batch->bits != lf->bits) throw std::runtime_error("[LogoFind] surfaces of another depth than the finder's");
        // a Y plane is a Y plane whatever the chroma layout; the MSB form (shift 0 at 16 bits: the plain one) reads container >> shift
        logofind_add(lf, b, nframes);
    });
}

int64_t amtgpu_logofind_nframes(const AmtGpuLogoFind* lf) { return lf ? lf->nframes : -1; }

int amtgpu_logofind_get_sums(AmtGpuLogoFind* lf, int64_t* sums)
{
    if (!lf) return 0;
    return guard(lf->ctx, [&] {
        if (!sums) throw std::runtime_error("[LogoFind] null sums pointer");
        const std::vector<int64_t> h = logofind_pull(lf);
        std::memcpy(sums, h.data(), h.size() * sizeof(int64_t));
    });
}

int amtgpu_logofind_set_sums(AmtGpuLogoFind* lf, const int64_t* sums, int64_t nframes)
{
    if (!lf) return 0;
    return guard(lf->ctx, [&] {
        if (!sums) throw std::runtime_error("[LogoFind] null sums pointer");
        if (nframes < 0) throw std::runtime_error("[LogoFind] negative frame count");
        logofind_push(lf, sums, nframes);
    });
}

int amtgpu_logofind_candidates(AmtGpuLogoFind* lf, const AmtGpuLogoFindParams* params, AmtGpuLogoRect* out, int cap, int* ncand)
{
    if (!lf) return 0;
    return guard(lf->ctx, [&] {
        if (!ncand || cap < 0 || (cap > 0 && !out)) throw std::runtime_error("[LogoFind] bad output arguments");
        const std::vector<int64_t> h = logofind_pull(lf);
        if (!amtgpu_logofind_candidates_host(h.data(), lf->width, lf->height, lf->bits, lf->nframes, params, out, cap, ncand))
            throw std::runtime_error("[LogoFind] invalid detection parameters");
    });
}

int amtgpu_logofind_allreduce(AmtGpuLogoFind* lf, const AmtGpuCollectives* coll)
{
    if (!lf) return 0;
    return guard(lf->ctx, [&] {
        if (!coll) throw std::runtime_error("[LogoFind] null collectives");
        ShardGuard sg(coll, nullptr, "logo detection");
        logofind_reduce(lf, sg);
    });
}

int amtgpu_scanlogo_auto_bits(AmtGpuContext* c, const void* dY, const void* dU, const void* dV, int64_t strideY, int64_t strideUV, int pitchY,
                              int pitchUV, int imgw, int imgh, int bits, int nframes, int serviceid, const char* dstpath, int thy, int numMaxFrames,
                              AMTGPU_LOGO_ANALYZE_CB cb, const AmtGpuLogoFindParams* params, AmtGpuLogoRect* found)
{
    if (!c) return 0;
    zero_found(found);
    AmtGpuLogoRect r{};
    const int ok = guard(c, [&] {
        // what amtgpu_scanlogo_bits refuses about the planes, as far as the detection reads them: the luma plane alone
        const FrameBatch luma = plane_batch(bits, dY, nullptr, nullptr, strideY, 0, pitchY, 0, PlaneRules::ScanLogo);
        std::unique_ptr<AmtGpuLogoFind> lf(logofind_new(c, imgw, imgh, bits));
        logofind_add(lf.get(), luma, nframes);
        r = best_rect(lf.get(), params);
    });
    if (!ok) return 0;
    if (found) *found = r;
    return amtgpu_scanlogo_bits(c, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, imgw, imgh, bits, nframes, serviceid, dstpath, r.imgx, r.imgy,
                                r.w, r.h, thy, numMaxFrames, cb);
}

int amtgpu_scanlogo_auto(AmtGpuContext* c, const void* dY, const void* dU, const void* dV, int64_t strideY, int64_t strideUV, int pitchY,
                         int pitchUV, int imgw, int imgh, int nframes, int serviceid, const char* dstpath, int thy, int numMaxFrames,
                         AMTGPU_LOGO_ANALYZE_CB cb, const AmtGpuLogoFindParams* params, AmtGpuLogoRect* found)
{
    return amtgpu_scanlogo_auto_bits(c, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, imgw, imgh, 8, nframes, serviceid, dstpath, thy,
                                     numMaxFrames, cb, params, found);
}

int amtgpu_scanlogo_auto_sharded_bits(AmtGpuContext* c, const AmtGpuCollectives* coll, const void* dY, const void* dU, const void* dV,
                                      int64_t strideY, int64_t strideUV, int pitchY, int pitchUV, int imgw, int imgh, int bits, int nframes_local,
                                      int serviceid, const char* dstpath, int thy, int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb,
                                      const AmtGpuLogoFindParams* params, AmtGpuLogoRect* found)
{
    if (!c) return 0;
    zero_found(found);
    AmtGpuLogoRect r{};
    const int ok = guard(c, [&] {
        (void)scan_sample_bytes(bits);       // (the depth is the same on every rank)
        std::unique_ptr<AmtGpuLogoFind> lf(logofind_new(c, imgw, imgh, bits));
        ShardGuard sg(coll, nullptr, "logo detection");
        sg.attempt([&] {
            logofind_add(lf.get(), plane_batch(bits, dY, nullptr, nullptr, strideY, 0, pitchY, 0, PlaneRules::ScanLogo), nframes_local);
        });
        logofind_reduce(lf.get(), sg);
        r = best_rect(lf.get(), params);       // identical sums on every rank: the same answer (or the same "no logo found") everywhere
    });
    if (!ok) return 0;
    if (found) *found = r;
    return amtgpu_scanlogo_sharded_bits(c, coll, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, imgw, imgh, bits, nframes_local, serviceid,
                                        dstpath, r.imgx, r.imgy, r.w, r.h, thy, numMaxFrames, cb);
}

int amtgpu_scanlogo_auto_sharded(AmtGpuContext* c, const AmtGpuCollectives* coll, const void* dY, const void* dU, const void* dV, int64_t strideY,
                                 int64_t strideUV, int pitchY, int pitchUV, int imgw, int imgh, int nframes_local, int serviceid,
                                 const char* dstpath, int thy, int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb, const AmtGpuLogoFindParams* params,
                                 AmtGpuLogoRect* found)
{
    return amtgpu_scanlogo_auto_sharded_bits(c, coll, dY, dU, dV, strideY, strideUV, pitchY, pitchUV, imgw, imgh, 8, nframes_local, serviceid,
                                             dstpath, thy, numMaxFrames, cb, params, found);
}

// pass 1 over the raw clip ('AMTR' or 'AMTH'): the Y planes only, chunk by chunk through the pinned upload path; pass 2 is amtgpu_scanlogo_file itself
int amtgpu_scanlogo_file_auto(AmtGpuContext* c, const char* srcpath, int serviceid, const char* workfile, const char* dstpath, int thy,
                              int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb, const AmtGpuLogoFindParams* params, AmtGpuLogoRect* found)
{
    if (!c) return 0;
    zero_found(found);
    AmtGpuLogoRect r{};
    const int ok = guard(c, [&] {
        ShardGuard one(nullptr, cb);
        RawClipReader in(c, srcpath, true);
        std::unique_ptr<AmtGpuLogoFind> lf(logofind_new(c, in.hd.width, in.hd.height, in.hd.bits));
        while (in.next()) {
            logofind_add(lf.get(), luma_batch_unchecked(in.hd.bits, in.dY, (int64_t)in.ysz, in.hd.width), in.n);
            one.progress(0.f, in.nread, in.hd.frames, 0);
        }
        r = best_rect(lf.get(), params);
    });
    if (!ok) return 0;
    if (found) *found = r;
    return amtgpu_scanlogo_file(c, srcpath, serviceid, workfile, dstpath, r.imgx, r.imgy, r.w, r.h, thy, numMaxFrames, cb);
}

} // extern "C"
