// amt_gpu_deband.hip -- C ABI part 8: the deband behind the temporal NR in the server's chain (KDeband(25, 1, 2, true), Misc.cs:1431;
// the GUI's "banding reduction" checkbox) over frames resident in HBM ("parity unpinned").  The object holds the
// three planes' offset tables (deband_plan.hpp) on the host, as the caller sees them, and on the device, rows padded to 16 entries
// with zeros, which is how the kernel loads them, and there also the U and V tables interleaved, for surfaces whose UV plane is one plane.
// Two entry points over one set of argument checks: amtgpu_deband_run takes planar LSB planes and nothing else;
// amtgpu_deband_run_surfaces takes every pair of descriptors in kind and runs the rule on samples (container >> shift in, result <<
// shift out).
#include "build_knobs.h"
#include "../../include/amt_gpu.h"

#include <memory>
#include <string>

#include "api_common.hpp"
#include "plane_pair.hpp"
#include "deband_plan.hpp"

using namespace amt;

static_assert(kDebandHalo == kDebandMaxRadius, "the kernel's halo is the plan's largest radius");

struct AmtGpuDeband {
    AmtGpuContext* ctx;
    int width, height, bits, radius, threshold, sample, blur_first;
    DebandTable table[3];                      // Y, U, V
    int table_pitch[3];                        // device rows: the plane's width rounded up to 16
    size_t table_at[3][2];                     // where a plane's dx / dy begin in dTables
    int uv_pitch;                              // the interleaved UV table's rows: width rounded up to 16, height / 2 of them
    size_t uv_at[2];                           // where its dx / dy begin in dTables: U's entry at 2x, V's at 2x + 1
    DevBuf<int8_t> dTables;
};

namespace {
const PlanePairRule& kPair = kDebandPair;
const char* const kWho = kPair.who;

[[noreturn]] void refuse(const std::string& what) { throw std::runtime_error(std::string(kWho) + " " + what); }

// one plane's table to the device, rows padded with zeros
void upload_table(AmtGpuDeband* d, int plane)
{
    const DebandTable& t = d->table[plane];
    const int pitch = d->table_pitch[plane];
    std::vector<int8_t> padded((size_t)pitch * t.H, 0);
    AmtGpuContext* c = d->ctx;
    c->bind();
    AMT_HIP(hipStreamSynchronize(c->stream));            // no launch still reads the table this replaces
    for (int k = 0; k < 2; ++k) {
        const std::vector<int8_t>& v = k ? t.dy : t.dx;
        for (int y = 0; y < t.H; ++y) std::copy(v.begin() + (size_t)y * t.W, v.begin() + (size_t)(y + 1) * t.W, padded.begin() + (size_t)y * pitch);
        AMT_HIP(hipMemcpyAsync(d->dTables.get() + d->table_at[plane][k], padded.data(), padded.size(), hipMemcpyHostToDevice, c->stream));
        AMT_HIP(hipStreamSynchronize(c->stream));        // `padded` is refilled, then freed
    }
}

// the interleaved UV table, from the host's U and V tables
void upload_interleaved(AmtGpuDeband* d)
{
    const DebandTable &u = d->table[1], &v = d->table[2];
    AmtGpuContext* c = d->ctx;
    c->bind();
    AMT_HIP(hipStreamSynchronize(c->stream));            // no launch still reads the table this replaces
    for (int k = 0; k < 2; ++k) {
        const std::vector<int8_t> both = deband_interleave(k ? u.dy : u.dx, k ? v.dy : v.dx, u.W, u.H, d->uv_pitch);
        AMT_HIP(hipMemcpyAsync(d->dTables.get() + d->uv_at[k], both.data(), both.size(), hipMemcpyHostToDevice, c->stream));
        AMT_HIP(hipStreamSynchronize(c->stream));        // `both` is freed
    }
}

AmtGpuDeband* deband_create(AmtGpuContext* c, int width, int height, int bits, int radius, int threshold, int sample, int blur_first, uint32_t seed)
{
    if (width <= 0 || height <= 0 || ((width | height) & 1)) refuse("width and height must be even and positive (4:2:0)");
    if (width > kDebandMaxSize || height > kDebandMaxSize) refuse("sizes above 65534 are not supported (the offset hash packs y << 16 | x)");
    if (bits < 8 || bits > 16) refuse("bits must be 8..16");
    if (radius < 1 || radius > kDebandMaxRadius) refuse("radius must be 1..31");
    if (threshold < 0 || threshold > 32767) refuse("threshold must be 0..32767");
    if (sample < 0 || sample > 2) refuse("sample must be 0, 1 or 2");
    std::unique_ptr<AmtGpuDeband> d(new AmtGpuDeband{});
    d->ctx = c; d->width = width; d->height = height; d->bits = bits; d->radius = radius; d->threshold = threshold; d->sample = sample;
    d->blur_first = blur_first ? 1 : 0;
    size_t at = 0;
    for (int p = 0; p < 3; ++p) {
        const int W = p ? width / 2 : width, H = p ? height / 2 : height;
        d->table[p] = deband_table(p, W, H, deband_plane_radius(p, radius), seed);
        d->table_pitch[p] = (W + 15) & ~15;
        for (int k = 0; k < 2; ++k) { d->table_at[p][k] = at; at += (size_t)d->table_pitch[p] * H; }
    }
    d->uv_pitch = (width + 15) & ~15;
    for (int k = 0; k < 2; ++k) { d->uv_at[k] = at; at += (size_t)d->uv_pitch * (height / 2); }
    c->bind();
    d->dTables.alloc(at);
    for (int p = 0; p < 3; ++p) upload_table(d.get(), p);
    upload_interleaved(d.get());
    return d.release();
}

// both entry points: any_layout is amtgpu_deband_run_surfaces, which takes every pair in kind
void deband_run(AmtGpuDeband* d, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes, bool any_layout)
{
    AmtGpuContext* c = d->ctx;
    if (nframes < 0) refuse("negative frame count");
    if (nframes == 0) return;
    // the source/destination rule (plane_pair.hpp)
    const FrameBatch s = kPair.side("source", src, surface_batch(src, kWho), d->width, any_layout, d->bits),
                     t = kPair.side("destination", dst, surface_batch(dst, kWho), d->width, any_layout, d->bits);
    kDebandPair.in_kind(s, t);                           // (planar LSB sides are in kind)
    const PlaneBytes sb = kPair.bytes(s, d->width, d->height), tb = kPair.bytes(t, d->width, d->height);
    kPair.disjoint(sb, nframes, tb, nframes);

    const int vec = deband_vec16(sb.luma(), sb.chroma(), tb.luma(), tb.chroma());
    const int thresh = d->threshold << (d->bits - 8);    // counts samples
    auto table = [&](int p, int k) { return d->dTables.get() + d->table_at[p][k]; };
    c->bind();
    if (!s.interleaved && !s.shift) {
        // planar LSB planes: the planar kernel, as before
        DebandArgs a{};
        for (int p = 0; p < 3; ++p) {
            const int k = p ? 1 : 0;
            a.plane[p] = DebandPlaneArgs{(const uint8_t*)sb.p[p], (uint8_t*)tb.p[p], table(p, 0), table(p, 1),
                                         sb.stride[k], tb.stride[k], sb.pitch[k], tb.pitch[k], d->table[p].W, d->table[p].H, d->table[p].R, d->table_pitch[p]};
        }
        a.es = s.es; a.vec = vec; a.thresh = thresh;
        a.sample = d->sample; a.blur_first = d->blur_first;
        const int sp_ = c->prof_begin("deband_kernel");
        AMT_HIP(launch_deband(c->stream, a, nframes));
        c->prof_end(sp_);
    } else {
        DebandSurfaceArgs a{};
        a.nplanes = sb.nplanes;
        for (int p = 0; p < sb.nplanes; ++p) {
            const int k = p ? 1 : 0;
            const DebandTable& tp = d->table[p];
            const bool uv = p && s.interleaved;          // one plane of `width` containers, 2 containers to a unit of a horizontal offset
            a.plane[p] = DebandSurfacePlaneArgs{(const uint8_t*)sb.p[p], (uint8_t*)tb.p[p], uv ? d->dTables.get() + d->uv_at[0] : table(p, 0),
                                                uv ? d->dTables.get() + d->uv_at[1] : table(p, 1), sb.stride[k], tb.stride[k], sb.pitch[k], tb.pitch[k],
                                                uv ? 2 * tp.W : tp.W, tp.H, uv ? 2 * tp.R : tp.R, tp.R, uv ? d->uv_pitch : d->table_pitch[p]};
        }
        a.es = s.es; a.vec = vec; a.shift = s.shift; a.thresh = thresh;
        a.sample = d->sample; a.blur_first = d->blur_first;
        const int sp_ = c->prof_begin("deband_surface_kernel");
        AMT_HIP(launch_deband_surfaces(c->stream, a, nframes));
        c->prof_end(sp_);
    }
    AMT_HIP(hipStreamSynchronize(c->stream));            // as amtgpu_resize_run: dst is ready when the call returns
}

const DebandTable& table_of(AmtGpuDeband* d, int plane)
{
    if (plane < 0 || plane > 2) refuse("plane is 0 (Y), 1 (U) or 2 (V)");
    return d->table[plane];
}

void deband_get_offsets(AmtGpuDeband* d, int plane, int8_t* dx, int8_t* dy)
{
    const DebandTable& t = table_of(d, plane);
    if (dx) std::copy(t.dx.begin(), t.dx.end(), dx);
    if (dy) std::copy(t.dy.begin(), t.dy.end(), dy);
}

void deband_set_offsets(AmtGpuDeband* d, int plane, const int8_t* dx, const int8_t* dy)
{
    table_of(d, plane);
    if (!dx || !dy) refuse("null offset table");
    DebandTable& t = d->table[plane];
    const long long bad = deband_first_offset_outside(dx, dy, t.W, t.H, t.R);
    if (bad >= 0)
        refuse("offset (" + std::to_string((int)dx[bad]) + ", " + std::to_string((int)dy[bad]) + ") at x " + std::to_string(bad % t.W) + ", y " + std::to_string(bad / t.W) +
               " of plane " + std::to_string(plane) + " exceeds lim(x, y) = " + std::to_string(deband_lim((int)(bad % t.W), (int)(bad / t.W), t.W, t.H, t.R)) +
               ": a reference would lie outside the plane");
    t.dx.assign(dx, dx + t.dx.size());
    t.dy.assign(dy, dy + t.dy.size());
    upload_table(d, plane);
    if (plane) upload_interleaved(d);
}
} // namespace

extern "C" {

AmtGpuDeband* amtgpu_deband_create(AmtGpuContext* c, int width, int height, int bits, int radius, int threshold, int sample, int blur_first, uint32_t seed)
{
    if (!c) return nullptr;
    AmtGpuDeband* d = nullptr;
    guard(c, [&] { d = deband_create(c, width, height, bits, radius, threshold, sample, blur_first, seed); });
    return d;
}

void amtgpu_deband_destroy(AmtGpuDeband* d) { delete d; }

int amtgpu_deband_run(AmtGpuDeband* d, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes)
{
    if (!d) return 0;
    return guard(d->ctx, [&] { deband_run(d, src, dst, nframes, false); });
}

int amtgpu_deband_run_surfaces(AmtGpuDeband* d, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes)
{
    if (!d) return 0;
    return guard(d->ctx, [&] { deband_run(d, src, dst, nframes, true); });
}

int amtgpu_deband_get_offsets(AmtGpuDeband* d, int plane, int8_t* dx, int8_t* dy)
{
    if (!d) return 0;
    return guard(d->ctx, [&] { deband_get_offsets(d, plane, dx, dy); });
}

int amtgpu_deband_set_offsets(AmtGpuDeband* d, int plane, const int8_t* dx, const int8_t* dy)
{
    if (!d) return 0;
    return guard(d->ctx, [&] { deband_set_offsets(d, plane, dx, dy); });
}

} // extern "C"
