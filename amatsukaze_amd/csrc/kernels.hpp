// kernels.hpp -- the interface between the kernel files (*_kernels.hip) and the host code that launches them: every launcher is declared
// here and nowhere else (default arguments too), and so is every struct both sides see.  Each kernel file includes it, so a definition
// that has drifted from its declaration, or a second definition of a struct passed by value into a kernel, does not compile.
// (The entries of stats_msb_kernels.hip and logofind_msb_kernels.hip, which only launch_frame_stats and launch_logofind call, are in their body headers.)
// A batch of frames crosses it as one struct in one unit convention (FrameBatch: frame strides in bytes; null chroma for the passes that read
// the Y plane alone), and the lane widths the copy-shaped launchers choose come from one rule (lane_rule.h; the weave's vec flag is still
// formed in amt_gpu_ingest.hip).
// Kept light on purpose (no <vector>, <string>, <mutex>): it goes into translation units that are all device code.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "eval_plan.h"
#include "frame_batch.h"
#include "lane_rule.h"
#include "resize_region.h"

namespace amt {

struct TileDesc; struct TileBandDesc;     // eval_tiles.hpp

// ---- descriptors ----
// (FrameBatch, the one description of a batch of frames every launcher takes, and plane_batch_from: frame_batch.h)
// the planes Delogo writes: laid out like the FrameBatch it reads (the same planes for the in-place call)
struct PlanesOut { void *Y, *U, *V; };
// a 4:2:0 rectangle of a frame: origin and size in the luma plane, and in the chroma planes
struct ScanRect { int imgx, imgy, cx, cy, w, h, wUV, hUV; };
inline ScanRect scan_rect(int imgx, int imgy, int w, int h) { return ScanRect{imgx, imgy, imgx >> 1, imgy >> 1, w, h, w >> 1, h >> 1}; }

// f(pix_t()) with the sample type of a clip `bits` deep: a launcher writes its kernel's argument list once, in a generic lambda
template <typename F> inline void with_sample_type(int bits, F&& f) { bits <= 8 ? f(uint8_t()) : f(uint16_t()); }

// ---- erase_scan_kernels.hip ----
struct EraseGeom {
    int w, h, wUV, hUV;
    int imgx, imgy, cx, cy;       // rectangle origin in luma / chroma planes
    int uvparity;
};
hipError_t launch_delogo(hipStream_t st, int bits, const FrameBatch& src, const PlanesOut& dst, const float* dplanes, EraseGeom g, int nframes,
                         const float2* dfades, int zero_identity);
// erase_surface_kernels.hip: the same Delogo on decoder surfaces where they lie (interleaved and / or MSB-aligned; planar LSB batches go to
// launch_delogo, which refuses every other); dst is laid out like src (the same planes for the in-place call)
hipError_t launch_delogo_surfaces(hipStream_t st, int bits, const FrameBatch& src, const PlanesOut& dst, const float* dplanes, EraseGeom g,
                                  int nframes, const float2* dfades, int zero_identity);
hipError_t launch_calc_fades(hipStream_t st, const float* danalysis, int analysis_first, int analysis_count, int num_frames, int first,
                             int nframes, const uint8_t* dstate, int half, float2* dout);
// (these three and launch_delogo take planar LSB batches; any other is hipErrorInvalidValue)
// dout[frame] = {valid, bgY, bgU, bgV}
hipError_t launch_scan_border(hipStream_t st, int bits, const FrameBatch& b, const ScanRect& r, int thy, int nframes, int4* dout);
// daccepted[i] = {frame, bgY, bgU, bgV}; dacc: 3 int64 per sample of the rectangle, added to
hipError_t launch_scan_accumulate(hipStream_t st, int bits, const FrameBatch& b, const ScanRect& r, const int4* daccepted, int naccepted,
                                  unsigned long long* dacc);
// the rectangle r of frames dkeep[0 .. nkeep) of a planar LSB batch (batch-local indices) into slots first_slot .. of a tight
// store: Y [slot][h][w], U / V [slot][hUV][wUV] samples.  Plane bases (batch and store) are multiples of es.  One launch; none when
// nkeep <= 0
hipError_t launch_scan_keep(hipStream_t st, const FrameBatch& b, const ScanRect& r, const int* dkeep, int nkeep, const PlanesOut& store,
                            long long first_slot);

// ---- surface_kernels.hip ----
// the rectangle r of all nframes surfaces as planar LSB samples: w x h luma at dst.Y, wUV x hUV chroma at dst.U / dst.V per frame (strides
// in bytes, pitches in samples).  Plane bases are multiples of es.  One launch
hipError_t launch_surfaces_extract(hipStream_t st, const FrameBatch& s, const ScanRect& r, int nframes, const PlanesOut& dst, long long dstrideY,
                                   long long dstrideUV, int dpitchY, int dpitchUV);

// ---- ingest_kernels.hip ----
struct WeaveArgs {
    const uint8_t* srcY; const uint8_t* srcU; const uint8_t* srcV;   // decoded pictures (srcV unused for NV12)
    long long src_strideY, src_strideUV;                             // bytes between pictures
    int src_pitchY, src_pitchUV;                                     // bytes per source row
    uint8_t* dstY; uint8_t* dstU; uint8_t* dstV;
    long long dst_strideY, dst_strideUV;
    int dst_pitchY, dst_pitchUV;                                     // bytes
    int rowY, rowUV;                                                 // bytes per output row (width * es, widthUV * es)
    int H, HUV;
    int nv12, es, vec;                                               // vec: all rows 16-byte aligned
    int shift = 0;                                                   // MSB-aligned pictures (es 2): sample = container >> shift
};
// a.shift != 0 launches the kernel's shifting form; the plain copy is the same code as before
hipError_t launch_weave_fields(hipStream_t st, const WeaveArgs& a, const int* dtop_index, const int* dbottom_index, int nframes);
// `nchunks` pieces of `chunk` bytes, src_stride apart at src (HBM, or page-locked host memory at its device address), dst_stride apart at dst
hipError_t launch_ingest_rows(hipStream_t st, const void* src, long long src_stride, void* dst, long long dst_stride, unsigned long long chunk,
                              long long nchunks);

// ---- render_kernels.hip ----
// One output frame of the cadence renderer as the kernel reads it, batch-local picture numbers: kind 0 weaves even
// rows of `top` with odd rows of `bottom`; kinds 1 / 2 (top == bottom == n) keep the even / odd rows of n and interpolate the others, with
// `other` the picture that holds the missing rows' second temporal neighbour (n - 1 for kind 1, n + 1 for kind 2; n itself at the clip's
// ends and wherever thresh < 0, so that nothing else is ever addressed)
struct RenderEntry { int kind, top, bottom, other; };
struct RenderArgs {
    const uint8_t *srcY, *srcU, *srcV; uint8_t *dstY, *dstU, *dstV;
    long long src_strideY, src_strideUV, dst_strideY, dst_strideUV;  // bytes between pictures
    int src_pitchY, src_pitchUV, dst_pitchY, dst_pitchUV;            // bytes between rows
    int rowY, rowUV;                                                 // bytes per row that are samples (width * es, width / 2 * es)
    int H, HUV;
    int es, vec;                                                     // vec: every base, stride and pitch is a multiple of 16 bytes
    int thresh;                                                      // < 0: no temporal neighbour is read; else clamped to the container's range
};
// nout output frames from dplan (device, nout entries).  One launch; none when nout <= 0
hipError_t launch_kfm_render(hipStream_t st, const RenderArgs& a, const RenderEntry* dplan, int nout);
// render_surface_kernels.hip: the same frames on decoder surfaces, source and destination in kind (planar LSB surfaces are ordinary planes
// and go to launch_kfm_render).  interleaved: srcU / dstU are the UV planes, a.rowUV their width * es bytes, srcV / dstV unused.
// shift != 0 (es 2): MSB-aligned containers; interpolated samples are container >> shift, stored << shift, and a.thresh counts samples
hipError_t launch_kfm_render_surfaces(hipStream_t st, const RenderArgs& a, int interleaved, int shift, const RenderEntry* dplan, int nout);
// render_adaptive_kernels.hip: the same frames on planar LSB planes with the bobs' missing rows from the edge-directed, motion-adaptive
// rule.  A bob entry reads both neighbours of n: prev / next are n - 1 / n + 1, batch-local, and n itself where the
// clip has none (and in WEAVE entries), so that nothing else is ever addressed.  a.thresh is not read
struct RenderAdaptiveEntry { int kind, top, bottom, prev, next; };
hipError_t launch_kfm_render_adaptive(hipStream_t st, const RenderArgs& a, const RenderAdaptiveEntry* dplan, int nout);
// render_adaptive_surface_kernels.hip: the adaptive rule on decoder surfaces, source and destination in kind; interleaved and shift as for
// launch_kfm_render_surfaces.  U and V of an interleaved plane are planes of their own (neighbours two containers away, the column clamp
// per component); interpolated samples are container >> shift, stored << shift.  Planar LSB planes (neither) are refused: they are
// launch_kfm_render_adaptive's
hipError_t launch_kfm_render_adaptive_surfaces(hipStream_t st, const RenderArgs& a, int interleaved, int shift, const RenderAdaptiveEntry* dplan, int nout);

// ---- temporal_nr_kernels.hip ----
// The reference's TemporalNRFilter (VideoFilter.hpp:156-211) on planar LSB planes.  Output frame t (0 .. nout - 1) averages, per luma
// pixel, the window frames min(max(first + t + k, lo), hi), k = -d .. d, that lie within thresh of the centre frame first + t; all frame
// numbers are batch-local, lo / hi those of the clip's first and last frame (lo <= 0; the caller has checked that every window frame is
// inside the batch)
struct TemporalNRArgs {
    const uint8_t *srcY, *srcU, *srcV; uint8_t *dstY, *dstU, *dstV;
    long long src_strideY, src_strideUV, dst_strideY, dst_strideUV;  // bytes between frames
    int src_pitchY, src_pitchUV, dst_pitchY, dst_pitchUV;            // bytes between rows
    int W, H;                                                        // luma size in containers; both even, H % 4 == 0 when interlaced
    int es, vec;                                                     // vec: temporal_nr_vec16 (lane_rule.h)
    int d, thresh, interlaced;                                       // thresh: threshold << (bits - 8)
    int first, lo, hi;
};
// The grid of both launchers below: a cell is one lane's columns (16 bytes where a.vec, else two) of a chroma row and of the two luma
// rows that map to it, a block 256 consecutive cells of one output frame.  False where an argument or the grid is out of range
struct TemporalNRGrid { int cells_per_row, blocks_per_frame; unsigned blocks; };
inline bool temporal_nr_grid(const TemporalNRArgs& a, int nout, TemporalNRGrid& g)
{
    if ((a.es != 1 && a.es != 2) || a.d < 0 || a.d > 63 || a.W <= 0 || a.H <= 0 || (a.W & 1) || (a.H & 1)) return false;
    const int px = a.vec ? 16 / a.es : 2;
    const long long cells_per_row = (a.W + px - 1) / px, cells = cells_per_row * (a.H >> 1);
    const long long blocks_per_frame = (cells + 255) / 256;
    if (cells > 0x7FFFFF00LL || blocks_per_frame * nout > 0x7FFFFFFFLL) return false;
    g = TemporalNRGrid{(int)cells_per_row, (int)blocks_per_frame, (unsigned)(blocks_per_frame * nout)};
    return true;
}
// One launch; none when nout <= 0.  The cell both kernel files instantiate is temporal_nr_body.h's
hipError_t launch_temporal_nr(hipStream_t st, const TemporalNRArgs& a, int nout);
// temporal_nr_surface_kernels.hip: the same frames on decoder surfaces, source and destination in kind (planar LSB planes -- neither
// interleaved nor shift -- are refused: they are the launcher's above).  interleaved: srcU / dstU are the UV planes, U the even and V the
// odd container of a row, srcV / dstV unused.  shift != 0 (es 2): MSB-aligned containers; the rule runs on container >> shift, a.thresh
// counts samples, and every container is stored as result << shift.  a.vec: temporal_nr_surface_vec16 (lane_rule.h)
hipError_t launch_temporal_nr_surfaces(hipStream_t st, const TemporalNRArgs& a, int interleaved, int shift, int nout);

// ---- resize_kernels.hip ----
// The resize of DESIGN.md section 6e on planar LSB planes: two stages, horizontal into the caller's intermediate, then vertical, one
// launch each for luma and both chroma planes of all nframes frames.  A stage resamples the axis its programs describe
// (resize_plan.hpp, on the device): out[i] = clamp((sum_j coeff[i * K + j] * s[start[i] + j] + 8192) >> 14, 0, maxv), int32 throughout.
struct ResizeProgramDev { const int* start; const int* coeff; int S, D, K, pad_; };
struct ResizePlaneArgs {
    const uint8_t* src; uint8_t* dst;
    long long src_stride, dst_stride;          // bytes between frames
    int src_pitch, dst_pitch;                  // bytes between rows
};
constexpr int kResizeWaves = 4;                // waves of a workgroup; each works on its own
                                               // (kResizeRegionBytes, kResizeRegionSlack: a wave's LDS region, resize_region.h)
constexpr int kResizeRows = 16;               // rows a wave of the horizontal stage walks with its coefficients in registers
struct ResizeStageArgs {
    ResizePlaneArgs plane[3];                  // Y, U, V
    ResizeProgramDev prog[2];                  // luma, chroma: the axis this stage resamples
    int lines[2];                              // luma, chroma: the lines the stage resamples -- rows of the source (horizontal: its height),
                                               // columns of the intermediate (vertical: the destination's width)
    int cpw[2];                                // horizontal: output columns of a wave's run, 1..64 (resize_columns_per_wave)
    int es, vec, maxv;                         // vec: resize_vec16 (lane_rule.h)
};
// (a.cpw[] comes from resize_columns_per_wave, declared in resize_region.h and defined with the plan in resize_plan.cpp)
// One launch each; none when nframes <= 0.  a.plane[].src of the vertical stage is the horizontal stage's dst
hipError_t launch_resize_h(hipStream_t st, const ResizeStageArgs& a, int nframes);
hipError_t launch_resize_v(hipStream_t st, const ResizeStageArgs& a, int nframes);
// resize_surface_kernels.hip: the same stages on decoder surfaces, source and destination in kind (planar LSB planes -- neither
// interleaved nor shift -- are refused: they are the launchers' above; what the two files share, the four launchers' argument check
// and grids included, is resize_body.h).  The intermediate holds LSB samples.  interleaved: a frame is
// two planes, plane[0] = Y and plane[1] = UV, whose rows are pairs -- the horizontal stage's prog[1] and lines[1] are the chroma plane's
// as above and its cpw[1] is resize_pair_columns_per_wave's (1..32); the vertical stage's lines[1] is the UV row's containers, twice the
// chroma width.  shift = 16 - bits where MSB-aligned: the horizontal stage reads container >> shift, the vertical stage stores
// result << shift.  a.vec: resize_surface_vec16 (lane_rule.h)
hipError_t launch_resize_surfaces_h(hipStream_t st, const ResizeStageArgs& a, int interleaved, int shift, int nframes);
hipError_t launch_resize_surfaces_v(hipStream_t st, const ResizeStageArgs& a, int interleaved, int shift, int nframes);

// ---- deband_kernels.hip ----
// The deband of DESIGN.md section 6f on planar LSB planes: per pixel up to four references at the offsets a static table holds, every
// plane and every frame on its own.  A 256-thread workgroup owns a tile of kDebandTileW x kDebandTileH output samples of one plane of
// one frame and stages it, with the plane's radius of halo clipped to the plane, into LDS; a lane then takes 16 bytes of an output row.
constexpr int kDebandTileW = 128, kDebandTileH = 96;
constexpr int kDebandHalo = 31;                // the largest radius (deband_plan.hpp kDebandMaxRadius)
// Bytes between the staged rows of containers of es bytes: the tile and both halos, the up to 15 bytes by which the staged span begins
// in front of the halo (its first column is a multiple of 16 bytes), rounded up to 16 -- 208 and 400
constexpr int deband_lds_pitch(int es) { return ((kDebandTileW + 2 * kDebandHalo) * es + 15 + 15) & ~15; }
// ... and of the staged rows: 32 864 and 63 200, so two workgroups of the 16-bit form share a CU's 160 KiB
constexpr int deband_lds_bytes(int es) { return deband_lds_pitch(es) * (kDebandTileH + 2 * kDebandHalo); }
struct DebandPlaneArgs {
    const uint8_t* src; uint8_t* dst;
    const int8_t *dx, *dy;                     // the plane's offsets, rows table_pitch bytes apart; |dx|, |dy| <= lim(x, y), which the
                                               // host has checked: a reference outside the staged span would be an LDS read out of bounds
    long long src_stride, dst_stride;          // bytes between frames
    int src_pitch, dst_pitch;                  // bytes between rows
    int W, H, R;                               // the plane's size in containers and its radius (0..kDebandHalo)
    int table_pitch;                           // a multiple of 16, at least W rounded up to 16: a lane loads its 16 / es entries at once
};
struct DebandArgs {
    DebandPlaneArgs plane[3];                  // Y, U, V
    int es, vec;                               // vec: deband_vec16 (lane_rule.h)
    int thresh;                                // threshold << (bits - 8)
    int sample, blur_first;                    // 0..2; zero or not
};
// The grid of the launcher below: x walks a frame's tiles, luma first, then U's, then V's; y the frames, a block taking every
// gridDim.y-th where there are more than 65 535.  False where an argument or the grid is out of range
struct DebandGrid { int tiles_x[2], tiles[2]; dim3 grid; };
inline bool deband_grid(const DebandArgs& a, int nframes, DebandGrid& g)
{
    if ((a.es != 1 && a.es != 2) || a.sample < 0 || a.sample > 2 || a.thresh < 0 || nframes <= 0) return false;
    for (int p = 0; p < 3; ++p) {
        const DebandPlaneArgs& q = a.plane[p];
        if (!q.src || !q.dst || !q.dx || !q.dy || q.W <= 0 || q.H <= 0 || q.W > 65534 || q.H > 65534 || q.R < 0 || q.R > kDebandHalo) return false;
        if (q.src_pitch < q.W * a.es || q.dst_pitch < q.W * a.es || q.table_pitch % 16 || q.table_pitch < ((q.W + 15) & ~15)) return false;
        if (p && (q.W != a.plane[1].W || q.H != a.plane[1].H)) return false;
    }
    for (int k = 0; k < 2; ++k) {
        g.tiles_x[k] = (a.plane[k].W + kDebandTileW - 1) / kDebandTileW;
        g.tiles[k] = g.tiles_x[k] * ((a.plane[k].H + kDebandTileH - 1) / kDebandTileH);
    }
    g.grid = dim3((unsigned)(g.tiles[0] + 2 * g.tiles[1]), (unsigned)(nframes < 65535 ? nframes : 65535));
    return true;
}
// One launch for all planes and frames; none when nframes <= 0
hipError_t launch_deband(hipStream_t st, const DebandArgs& a, int nframes);

// ---- deband_surface_kernels.hip ----
// The same rule on decoder surfaces in kind (NV12, interleaved 16-bit LSB, P010 / P012 / P016, planar 16-bit MSB), the planar kernel's
// shape: the same tile, LDS pitch and bytes.  nplanes 3: Y, U, V each a plane of its own.  nplanes 2 (interleaved): Y and the UV plane,
// which is walked as ONE plane of `width` containers by height / 2 rows whose table holds U's entry at 2x and V's at 2x + 1 and whose
// cell steps 2 containers per unit of a horizontal offset; it stages RX = 2 * (radius >> 1) columns and RY = radius >> 1 rows of halo
// where a plane of its own has RX = RY = its radius.  shift = 16 - bits where MSB-aligned: LDS holds container >> shift, the rule runs
// on those samples (thresh counts them), and every destination container is result << shift
static_assert(2 * (kDebandHalo >> 1) <= kDebandHalo, "the interleaved UV plane's column halo fits the planar kernel's LDS pitch");
struct DebandSurfacePlaneArgs {
    const uint8_t* src; uint8_t* dst;
    const int8_t *dx, *dy;                     // as DebandPlaneArgs; the interleaved UV plane's: the object's interleaved table
    long long src_stride, dst_stride;          // bytes between frames
    int src_pitch, dst_pitch;                  // bytes between rows
    int W, H;                                  // the plane's size in containers (the UV plane: width x height / 2)
    int RX, RY;                                // columns and rows of halo (0..kDebandHalo)
    int table_pitch;                           // a multiple of 16, at least W rounded up to 16
};
struct DebandSurfaceArgs {
    DebandSurfacePlaneArgs plane[3];           // Y, U, V or Y, UV (plane[2] is unused then)
    int nplanes;                               // 3, or 2: interleaved
    int es, vec;                               // vec: deband_vec16 (lane_rule.h) on both sides' planes
    int shift;                                 // 0, or 16 - bits of an MSB-aligned 16-bit surface
    int thresh;                                // threshold << (bits - 8), in samples
    int sample, blur_first;
};
// The grid, as deband_grid: x walks a frame's tiles, luma first, then the chroma plane's or planes'.  False where an argument or the grid
// is out of range
inline bool deband_surface_grid(const DebandSurfaceArgs& a, int nframes, DebandGrid& g)
{
    if ((a.es != 1 && a.es != 2) || a.sample < 0 || a.sample > 2 || a.thresh < 0 || nframes <= 0) return false;
    if ((a.nplanes != 2 && a.nplanes != 3) || a.shift < 0 || a.shift > 8 || (a.shift && a.es != 2)) return false;
    for (int p = 0; p < a.nplanes; ++p) {
        const DebandSurfacePlaneArgs& q = a.plane[p];
        if (!q.src || !q.dst || !q.dx || !q.dy || q.W <= 0 || q.H <= 0 || q.W > 65534 || q.H > 65534) return false;
        if (q.RX < 0 || q.RX > kDebandHalo || q.RY < 0 || q.RY > kDebandHalo) return false;
        if (q.src_pitch < q.W * a.es || q.dst_pitch < q.W * a.es || q.table_pitch % 16 || q.table_pitch < ((q.W + 15) & ~15)) return false;
        if (p && (q.W != a.plane[1].W || q.H != a.plane[1].H)) return false;
    }
    if (a.nplanes == 2 && (a.plane[1].W & 1)) return false;
    for (int k = 0; k < 2; ++k) {
        g.tiles_x[k] = (a.plane[k].W + kDebandTileW - 1) / kDebandTileW;
        g.tiles[k] = g.tiles_x[k] * ((a.plane[k].H + kDebandTileH - 1) / kDebandTileH);
    }
    g.grid = dim3((unsigned)(g.tiles[0] + (a.nplanes - 1) * g.tiles[1]), (unsigned)(nframes < 65535 ? nframes : 65535));
    return true;
}
// One launch for all planes and frames; none when nframes <= 0.  Planar LSB planes are not this launcher's: hipErrorInvalidValue
hipError_t launch_deband_surfaces(hipStream_t st, const DebandSurfaceArgs& a, int nframes);

// ---- edgelevel_kernels.hip ----
// The edge level of DESIGN.md section 6g on planar LSB planes: a luma stencil of five rows by five columns, chroma copied, every frame
// on its own.  A wave owns a strip of kEdgeStripRows output rows of one span of kEdgeSpanBytes bytes of the luma plane (a lane 16 of
// them) and slides a window of five rows down it; a block is four such waves, or four waves that each copy one chroma row.
constexpr int kEdgeStripRows = 32;
constexpr int kEdgeSpanBytes = 64 * 16;
struct EdgeLevelArgs {
    const uint8_t *srcY, *srcU, *srcV; uint8_t *dstY, *dstU, *dstV;
    long long src_strideY, src_strideUV, dst_strideY, dst_strideUV;  // bytes between frames
    int src_pitchY, src_pitchUV, dst_pitchY, dst_pitchUV;            // bytes between rows
    int W, H;                                                        // luma size in containers; both even
    int es, vec;                                                     // vec: edgelevel_vec16 (lane_rule.h)
    int strength, thresh, repair;                                    // 0..255; threshold << (bits - 8); 0..4
};
// The grid of the launcher below: x walks a frame's luma units (strip by strip, a strip's spans side by side), four to a block, then its
// chroma rows (U's, then V's), four to a block; y the frames, a block taking every gridDim.y-th where there are more than 65 535.  False
// where an argument or the grid is out of range
struct EdgeLevelGrid { int spans, units, luma_blocks; dim3 grid; };
inline bool edgelevel_grid(const EdgeLevelArgs& a, int nframes, EdgeLevelGrid& g)
{
    if ((a.es != 1 && a.es != 2) || a.W <= 0 || a.H <= 0 || (a.W & 1) || (a.H & 1) || nframes <= 0) return false;
    if (a.strength < 0 || a.strength > 255 || a.thresh < 0 || a.repair < 0 || a.repair > 4) return false;
    if (!a.srcY || !a.srcU || !a.srcV || !a.dstY || !a.dstU || !a.dstV) return false;
    if (a.src_pitchY < a.W * a.es || a.dst_pitchY < a.W * a.es || a.src_pitchUV < a.W / 2 * a.es || a.dst_pitchUV < a.W / 2 * a.es) return false;
    const long long spans = ((long long)a.W * a.es + kEdgeSpanBytes - 1) / kEdgeSpanBytes, strips = (a.H + kEdgeStripRows - 1) / kEdgeStripRows;
    const long long units = spans * strips, luma_blocks = (units + 3) / 4, chroma_blocks = (a.H + 3) / 4;    // H / 2 rows of U and of V
    if (units > 0x7FFFFFF0LL || luma_blocks + chroma_blocks > 0x7FFFFFFFLL) return false;
    g = EdgeLevelGrid{(int)spans, (int)units, (int)luma_blocks, dim3((unsigned)(luma_blocks + chroma_blocks), (unsigned)(nframes < 65535 ? nframes : 65535))};
    return true;
}
// One launch for all planes and frames; none when nframes <= 0.  The cell is edgelevel_body.h's
hipError_t launch_edgelevel(hipStream_t st, const EdgeLevelArgs& a, int nframes);

// ---- stats_kernels.hip, logofind_kernels.hip ----
// Both take a luma batch of either alignment: b.shift != 0 (16-bit containers, shift = 16 - bits) runs the same sums on container >> shift,
// `bits` then being the depth of the shifted samples (9..15 metrics, 9..16 finder): the instantiations of stats_msb_ / logofind_msb_kernels.hip.
hipError_t launch_frame_stats(hipStream_t st, int bits, const FrameBatch& b, int W, int H, const void* dprevY, int nframes, unsigned long long* dout);
// Largest frame count of one launch_logofind: its uint32 partials hold at most 2 * maxv per frame (SM) below 2^31.
long long logofind_launch_cap(int bits);
// nframes <= logofind_launch_cap(bits) (the caller splits); dS1 / dSM: W*H int64 each, added to
hipError_t launch_logofind(hipStream_t st, int bits, const FrameBatch& b, int W, int H, int nframes, int num_cus, unsigned long long* dS1,
                           unsigned long long* dSM);

// ---- audio_kernels.hip ----
// The audio timeline of a clip: video frame n owns sample-frames [b(n), b(n + 1)) below num_samples, b(n) = n * step_num / fps_num floored
// (step_num = sample_rate * fps_den); `channels` interleaved int16 elements per sample-frame
struct AudioTimeline { long long num_samples, step_num, fps_num; int channels; };
constexpr int kAudioLevelWords = 4;      // AMTGPU_AL_WORDS
// records of video frames [first_frame, first_frame + nframes) into dout (4 uint64 each); dpcm holds the timeline from sample-frame
// pcm_first on and covers every span of the range that is not empty (the caller has checked, and that (first_frame + nframes) * step_num
// fits 63 bits); 2-byte aligned, nothing more.  One launch; none when nframes <= 0
hipError_t launch_audio_levels(hipStream_t st, const int16_t* dpcm, long long pcm_first, const AudioTimeline& t, long long first_frame,
                               int nframes, unsigned long long* dout);

// ---- eval_fused_kernels.hip, eval_pair_kernels.hip, eval_linear_kernels.hip ----
// tile plan of one evaluation logo resident in HBM (eval_tiles.hpp; eval_pair_kernels.hip).  slot = (band * kTileWaves + wave) * 64 + lane
struct TileLogoDev {
    const float2* kp;            // [13][nslots]  taps of the slot's mask pixel as pairs {k[2j], k[2j+1]} (k[25] = 0), pair-major; times 0.25
                                 //               when the scan's pair kernel stages unscaled (EvalEngine::ensure_tiles)
    const float2* sc;            // [32][nslots]  bin-major {scale, scale2} of the slot's mask pixel (the exact scan kernel)
    const float2* pq;            // [nslots]      {P, Q}: the pixel's response on flat level c is |P + Q c| (the linear analysis kernel: no gathers)
    const uint32_t* sinfo;       // [nslots]      tile_slot_info
    const uint32_t* pos;         // [nslots]      (y << 16) | x of the slot's mask pixel in the evaluation logo (the linear kernel's exact bin check)
    const TileDesc* tiles;       // [nbands * 8]
    const TileBandDesc* bands;   // [nbands]
    const int* tlist;            // [ntlist]  indices of the tiles that hold pixels (kernels that need no band order walk these)
    int nbands, nslots, ntlist;
    float floorResp;             // limitCorr of the logo (LogoScan.hpp:203)
    // the linear kernel's copy of everything it loads per tile, in ONE allocation (one scalar base instead of five: its loop is short of
    // scalar registers): kp at 0, then pq, sinfo, the evaluation logo's a and b planes at these byte offsets
    const char* lin;
    unsigned lin_pq, lin_sinfo, lin_a, lin_b;
    // (new fields go here, at the end: the linear kernel reads the struct with scalar loads at fixed offsets)
    const uint32_t* units;       // [nslots]      tile_unit_word of the staging unit a lane holds, when the engine's plans are single-pass ones
                                 //               (eval_tiles.hpp kTileCutUnits; the scan's one-unit pair kernel); null otherwise
};
// These three and launch_rect_range_flag take a luma batch of LSB samples (a shift is hipErrorInvalidValue: surfaces_luma_view, api_common.hpp).
// eval_fused_kernels.hip.  dnframes (device, optional): the number of frames actually present (<= nframes,
// which then only sizes the grid); scatter != 0: frame i's results go to record dframe_map[i] of dout; fade_chunk > 0 (with dnframes):
// a workgroup evaluates fade_chunk of the fades, the chunks of a (logo, frame group) run side by side -- a handful of listed frames
// is a latency problem (one workgroup walking every band for all fades), not a throughput one
hipError_t launch_logo_eval_fused(hipStream_t st, int bits, const EvalLogoDev* dlogos, int nlogos, const EvalBand* dbands,
                                  const float* dfades, int nfades, int fade0, const FrameBatch& luma, const int* dframe_map, int nframes, int G,
                                  float* dout, int out_frame_stride, int take_abs, int plane_cap, const int* dnframes = nullptr, int scatter = 0,
                                  int fade_chunk = 0);
// eval_linear_kernels.hip
hipError_t launch_logo_eval_linear(hipStream_t st, int bits, const EvalLogoDev* dlogos, const TileLogoDev* dtls, int nlogos,
                                   const float* dfades, int nfades, int fade0, const FrameBatch& luma, const int* dframe_map, int nframes, int G,
                                   float* dout, int out_frame_stride, int take_abs, float bin_eps, int qlog2, int qcap, uint8_t* dforce);
// eval_pair_kernels.hip: fades {0, 1} of every logo, bit-exact
hipError_t launch_logo_eval_pair(hipStream_t st, int bits, const EvalLogoDev* dlogos, const TileLogoDev* dtls, int nlogos,
                                 const FrameBatch& luma, const int* dframe_map, int nframes, int G, float* dout, int out_frame_stride, int take_abs,
                                 int ldexp_form);
// eval_pair1_kernels.hip: the same on single-pass plans (every logo's TileLogoDev::units set), one staging unit per lane
hipError_t launch_logo_eval_pair1(hipStream_t st, int bits, const EvalLogoDev* dlogos, const TileLogoDev* dtls, int nlogos,
                                  const FrameBatch& luma, const int* dframe_map, int nframes, int G, float* dout, int out_frame_stride, int take_abs,
                                  int ldexp_form);
// eval_pair1_duo_kernels.hip: the same on single-pass plans of kPairDuoWaves tiles per band (eval_tiles.hpp tile_pair_shape), G <= kPairDuoFrames
hipError_t launch_logo_eval_pair1_duo(hipStream_t st, int bits, const EvalLogoDev* dlogos, const TileLogoDev* dtls, int nlogos,
                                      const FrameBatch& luma, const int* dframe_map, int nframes, int G, float* dout, int out_frame_stride, int take_abs,
                                      int ldexp_form);
// Sentinel monitor of AMTGPU_ANALYZE_LINEAR_MONITORED: persistent per-analyzer device state.  max_abs_bits: the largest |linear - exact| over
// every compared score as float bits (non-negative floats order like unsigned ints; NaN counts as +inf); tripped: a comparison failed (sticky
// until re-armed); frames_checked: sentinel frames compared; batches_tripped: batches in which a comparison failed
struct MonitorState {
    unsigned max_abs_bits;
    int tripped;
    unsigned long long frames_checked;
    unsigned batches_tripped;
    unsigned pad_;
};
// Sentinel arguments of the mark kernel (nsent = 0: none, the guarded mode).  The sentinels of a batch of nframes frames are
// s_j = floor(j (nframes - 1) / (nsent - 1)), j < nsent (nsent = 1: frame 0); nsent <= nframes.  side: [nsent][stride] copy of their
// linear records; side_forced: [nsent] their force byte; gate: [2] per-batch words the mark kernel zeroes (frames of the gated exact pass,
// workgroups that tripped) -- analysis_sentinel_check_kernel sets them, later launches read them
struct SentinelArgs {
    int nsent = 0;
    float* side = nullptr;
    uint8_t* side_forced = nullptr;
    int* gate = nullptr;
};
hipError_t launch_analysis_mark(hipStream_t st, const float* drec, int stride, int nframes, int ngroups, int nfades, const float* eps3,
                                int* dlist, int* dcount, const uint8_t* dforce = nullptr, const SentinelArgs& sent = SentinelArgs());
// compares the sentinels' exact records (rec, after the listed re-evaluation) with their saved linear copies; a failed comparison or an
// earlier one (state->tripped) sets gate[0] = nframes and stores `epoch` to the host-mapped word `host_flag` (optional)
hipError_t launch_analysis_sentinel_check(hipStream_t st, const float* drec, int stride, int nframes, const SentinelArgs& sent, float tol,
                                          MonitorState* dstate, int* host_flag, int epoch);
// list[i] = i for i < n (the identity list of the gated whole-batch re-evaluation)
hipError_t launch_analysis_iota(hipStream_t st, int* dlist, int n);
hipError_t launch_rect_range_flag(hipStream_t st, const FrameBatch& luma, int imgx, int imgy, int w, int h, int bits, int nframes, uint8_t* dflag);

} // namespace amt
