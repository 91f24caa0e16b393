// amt_gpu_deband.hip -- C ABI part 8: the deband behind the temporal NR in the server's chain (KDeband(25, 1, 2, true), Misc.cs:1431;
// the GUI's "banding reduction" checkbox) over frames resident in HBM ("parity unpinned").  The object holds the
// three planes' offset tables (deband_plan.hpp) on the host, as the caller sees them, and on the device, rows padded to 16 entries
// with zeros, which is how the kernel loads them.  Planar LSB planes and nothing else.
#include "build_knobs.h"
#include "../../include/amt_gpu.h"

#include <memory>
#include <string>

#include "api_common.hpp"
#include "deband_plan.hpp"

using namespace amt;

static_assert(kDebandHalo == kDebandMaxRadius, "the kernel's halo is the plan's largest radius");

struct AmtGpuDeband {
    AmtGpuContext* ctx;
    int width, height, bits, radius, threshold, sample, blur_first;
    DebandTable table[3];                      // Y, U, V
    int table_pitch[3];                        // device rows: the plane's width rounded up to 16
    size_t table_at[3][2];                     // where a plane's dx / dy begin in dTables
    DevBuf<int8_t> dTables;
};

namespace {
const char* const kWho = "[Deband]";

[[noreturn]] void refuse(const std::string& what) { throw std::runtime_error(std::string(kWho) + " " + what); }

// planar LSB surfaces of the object's bits with rows of at least width (chroma: width / 2) containers
FrameBatch deband_surfaces(const AmtGpuSurfaces* s, const char* which, int width, int bits)
{
    const FrameBatch b = surface_batch(s, kWho);
    if (s->interleaved || s->msb_aligned) refuse(std::string(which) + ": planar, LSB-aligned planes only (interleaved and MSB-aligned surfaces are refused)");
    if (s->bits != bits) refuse(std::string(which) + ": " + std::to_string(s->bits) + " bits, the debander was created for " + std::to_string(bits));
    if (b.strideY < 0 || b.strideUV < 0) refuse(std::string(which) + ": negative frame stride");
    if (b.pitchY < width || b.pitchUV < width / 2) refuse(std::string(which) + ": pitch smaller than the row");
    return b;
}

// [first byte, one past the last byte) that n frames of a plane span
struct Span { uintptr_t lo, hi; };
Span plane_span(const void* p, long long stride, long long pitch_bytes, int row_bytes, int rows, int n)
{
    const uintptr_t lo = (uintptr_t)p;
    return Span{lo, lo + (uintptr_t)(n - 1) * (uintptr_t)stride + (uintptr_t)(rows - 1) * (uintptr_t)pitch_bytes + (uintptr_t)row_bytes};
}

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
    c->bind();
    d->dTables.alloc(at);
    for (int p = 0; p < 3; ++p) upload_table(d.get(), p);
    return d.release();
}

void deband_run(AmtGpuDeband* d, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes)
{
    AmtGpuContext* c = d->ctx;
    if (nframes < 0) refuse("negative frame count");
    if (nframes == 0) return;
    const FrameBatch s = deband_surfaces(src, "source", d->width, d->bits), t = deband_surfaces(dst, "destination", d->width, d->bits);
    const int es = s.es;
    struct Geometry { int w, h; };
    const Geometry g[2] = {{d->width, d->height}, {d->width / 2, d->height / 2}};
    const long long s_stride[2] = {s.strideY, s.strideUV}, t_stride[2] = {t.strideY, t.strideUV};
    const long long s_pitch[2] = {(long long)s.pitchY * es, (long long)s.pitchUV * es}, t_pitch[2] = {(long long)t.pitchY * es, (long long)t.pitchUV * es};
    if (s_pitch[0] > INT32_MAX || s_pitch[1] > INT32_MAX || t_pitch[0] > INT32_MAX || t_pitch[1] > INT32_MAX) refuse("pitch above 2 GiB");
    const void* const sp[3] = {s.Y, s.U, s.V};
    const void* const tp[3] = {t.Y, t.U, t.V};
    // destination frames must not overlap each other, and no destination plane's span may touch a source plane's
    for (int k = 0; k < 2; ++k)
        if (nframes > 1 && t_stride[k] < (long long)(g[k].h - 1) * t_pitch[k] + (long long)g[k].w * es) refuse("destination frames overlap each other");
    Span sspan[3], dspan[3];
    for (int p = 0; p < 3; ++p) {
        const int k = p ? 1 : 0;
        sspan[p] = plane_span(sp[p], s_stride[k], s_pitch[k], g[k].w * es, g[k].h, nframes);
        dspan[p] = plane_span(tp[p], t_stride[k], t_pitch[k], g[k].w * es, g[k].h, nframes);
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (const Span &x = sspan[i], &y = dspan[j]; x.lo < y.hi && y.lo < x.hi)
                refuse("the destination's byte range overlaps the source's (no in-place filtering: the filter reads neighbours)");

    DebandArgs a{};
    for (int p = 0; p < 3; ++p) {
        const int k = p ? 1 : 0;
        a.plane[p] = DebandPlaneArgs{(const uint8_t*)sp[p], (uint8_t*)tp[p], d->dTables.get() + d->table_at[p][0], d->dTables.get() + d->table_at[p][1],
                                     s_stride[k], t_stride[k], (int)s_pitch[k], (int)t_pitch[k], g[k].w, g[k].h, d->table[p].R, d->table_pitch[p]};
    }
    const RowsAt srcY{lane_addr(s.Y), 0, s_stride[0], s_pitch[0]}, srcUV{lane_addr(s.U), lane_addr(s.V), s_stride[1], s_pitch[1]};
    const RowsAt dstY{lane_addr(t.Y), 0, t_stride[0], t_pitch[0]}, dstUV{lane_addr(t.U), lane_addr(t.V), t_stride[1], t_pitch[1]};
    a.es = es;
    a.vec = deband_vec16(srcY, srcUV, dstY, dstUV);
    a.thresh = d->threshold << (d->bits - 8);
    a.sample = d->sample; a.blur_first = d->blur_first;
    c->bind();
    const int sp_ = c->prof_begin("deband_kernel");
    AMT_HIP(launch_deband(c->stream, a, nframes));
    c->prof_end(sp_);
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
    return guard(d->ctx, [&] { deband_run(d, src, dst, nframes); });
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
