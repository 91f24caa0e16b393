/*
 * amt_gpu.h -- C ABI of the MI355X-native logo / CM / KFM analysis hot path.
 *
 * Drop-in boundary for the per-frame pixel analysis that nekopanda/Amatsukaze runs as scalar C++
 * inside Amatsukaze.dll.  Every entry point names the reference interface it replaces (paths relative
 * to the reference tree).  Conventions follow the reference's own exported C API
 * (LogoScan.hpp:1083-1098 ScanLogo, StreamUtils.hpp:1037-1039 AMTContext_*, LogoGUISupport.hpp:254-275):
 * opaque handles, int return 1 = ok / 0 = failure with the message kept on the context
 * (amtgpu_last_error), no exceptions across the boundary, handles freed by *_destroy.
 *
 * Frames are 4:2:0 planar, 8-bit (uint8) or 9..16-bit (uint16 containers), the layout AMTSource hands to
 * AviSynth (AMTSource.hpp:428-442).  A "batch" is `nframes` frames whose planes sit at
 * base + n*frame_stride (bytes); `pitch` is in ELEMENTS.  Pointers named d* are DEVICE pointers (HBM,
 * hipMalloc'ed by the caller or by amtgpu_frames_upload); everything else is host memory.
 *
 * All kernels are launched on the context's HIP stream (amtgpu_context_set_stream); calls that return
 * results to host memory synchronise that stream, calls documented "async" do not.
 * Calls on one context are serialised by a lock inside it (filters sharing a context may be driven from several
 * AviSynth threads); use one context per thread for concurrency.
 */
#ifndef AMT_GPU_H
#define AMT_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMTGPU_ABI_VERSION 5      /* 2: amtgpu_framestats_create lost two unused parameters; *W entry points, logo header access, markers
                                   * 3: additions only -- device-side CalcFade (amtgpu_erase_calc_fades_device, *_dfades), sharded frame
                                   *    metrics (amtgpu_framestats_allgather / _sharded), registered host frames (amtgpu_frames_register),
                                   *    amtgpu_download_scatter, owned markers
                                   * 4: amtgpu_logoframe_decide_host returns -1 (was 0) when the text buffer is too small and refuses
                                   *    num_candidates > num_logos; additions: amtgpu_logoframe_dump_result, amtgpu_host_set_parallelism
                                   * 5: amtgpu_logoframe_decide_host is back to 1 / 0 like every other entry point (a too-small text buffer
                                   *    is 0 with *text_len > cap: `if (!call) fail;` written against ABI <= 3 is right again); additions:
                                   *    amtgpu_analyze_set_fixup_queue, amtgpu_erase_batch_dfades_to
                                   * 5 (later additions): AMTGPU_ANALYZE_LINEAR_MONITORED, amtgpu_analyze_set_monitor,
                                   *    amtgpu_analyze_monitor_stats; automatic logo detection (amtgpu_logofind_*,
                                   *    amtgpu_scanlogo_auto, _auto_sharded, _file_auto); the streamed ScanLogo session
                                   *    (amtgpu_scanlogo_stream_*); ScanLogo for 9..12-bit clips (amtgpu_scanlogo_bits, _sharded_bits,
                                   *    _stream_create_bits, _auto_bits, _auto_sharded_bits; the 'AMTH' raw clip file); decoder surfaces
                                   *    (AmtGpuSurfaces: amtgpu_surfaces_extract_rect, amtgpu_scanlogo_stream_feed_surfaces,
                                   *    amtgpu_logofind_add_surfaces, amtgpu_weave_fields_batch_msb; amtgpu_erase_surfaces, _dfades, _dfades_to,
                                   *    amtgpu_analyze_surfaces, amtgpu_logoframe_scan_surfaces, amtgpu_framestats_surfaces,
                                   *    amtgpu_framestats_sharded_surfaces) */
#define AMTGPU_NUM_FADE 11            /* LogoAnalyzeFrame p/t/b[11]  (LogoScan.hpp:1100-1103) */
#define AMTGPU_ANALYZE_FLOATS 33      /* floats per source frame in an analysis record */

typedef struct AmtGpuContext AmtGpuContext;       /* AMTContext            (StreamUtils.hpp:343-511) */
typedef struct AmtGpuLogo AmtGpuLogo;             /* logo::LogoData+LogoHeader (AMTLogo.hpp:19-280) */
typedef struct AmtGpuLogoFrame AmtGpuLogoFrame;   /* logo::LogoFrame       (LogoScan.hpp:1521-1836) */
typedef struct AmtGpuAnalyze AmtGpuAnalyze;       /* logo::AMTAnalyzeLogo  (LogoScan.hpp:1106-1236) */
typedef struct AmtGpuErase AmtGpuErase;           /* logo::AMTEraseLogo    (LogoScan.hpp:1238-1519) */
typedef struct AmtGpuLogoScan AmtGpuLogoScan;     /* logo::LogoScan        (LogoScan.hpp:398-660) */
typedef struct AmtGpuFrameStats AmtGpuFrameStats; /* self-specified CM / KFM whole-frame metrics */

/* progress callback of ScanLogo (LogoScan.hpp:792): return 0 to cancel */
typedef int (*AMTGPU_LOGO_ANALYZE_CB)(float progress, int nread, int total, int ngather);

int amtgpu_abi_version(void);
/* Host threads of the O(frames) decision routines (selectLogo / writeResult text, scene changes, cadence): they cut the clip into
 * contiguous frame ranges -- the window filters are local -- and leave only the two small state machines sequential.  max_threads /
 * min_frames_per_thread <= 0 restore the defaults (half the host's cores up to 32; 32 768 frames).  Process-wide.  Results never depend
 * on either value.  A host with its own thread pool (AviSynth MT) passes 1 to keep the library on the calling thread. */
void amtgpu_host_set_parallelism(int max_threads, int min_frames_per_thread);
/* How many copies of the HIP runtime (libamdhip64) are mapped into this process, and where from (newline-separated paths in `paths`,
 * truncated to cap; may be NULL).  More than one -- e.g. this library bound to /opt/rocm's copy while another component brought its
 * own -- means device pointers and streams of one are unknown to the other: copies fail with "invalid argument", kernels fault.
 * A host that mixes ROCm users checks this once after loading everything (the Python mirror does, and loads torch first so that
 * both bind to the same copy). */
int amtgpu_hip_runtimes_loaded(char* paths, int cap);

/* ---- context: replaces AMTContext_Create / ATMContext_Delete / AMTContext_GetError
 *      (StreamUtils.hpp:1037-1039) ---- */
AmtGpuContext* amtgpu_context_create(int device);       /* NULL if no HIP device / bad index */
void           amtgpu_context_destroy(AmtGpuContext* ctx);
const char*    amtgpu_last_error(const AmtGpuContext* ctx);
/* use an existing hipStream_t (e.g. the caller's compute stream); NULL = the context's own stream, which is created
 * hipStreamNonBlocking: it is NOT ordered against the legacy default ("null") stream.  A caller whose other GPU work runs
 * on the null stream (handle 0, e.g. PyTorch without an explicit stream) passes AMTGPU_STREAM_LEGACY_DEFAULT
 * (== hipStreamLegacy) so that the "async" entry points below are stream-ordered with that work.  On any other stream
 * pair the caller orders the two with events or amtgpu_context_synchronize before consuming device outputs. */
#define AMTGPU_STREAM_LEGACY_DEFAULT ((void*)1)
int            amtgpu_context_set_stream(AmtGpuContext* ctx, void* hip_stream);
void*          amtgpu_context_get_stream(AmtGpuContext* ctx);
int            amtgpu_context_synchronize(AmtGpuContext* ctx);
/* Device partitions.  The whole-frame metrics are bandwidth work, the logo kernels arithmetic: run BESIDE each other they finish sooner
 * than one after the other -- but the hardware only co-schedules them when the device is partitioned (the logo kernels otherwise
 * take every CU's registers and LDS).  amtgpu_stream_create_cu_range returns a hipStream_t (hipStreamNonBlocking) whose kernels run on
 * `num_cus` compute units starting at `first_cu` in the driver's mask order, in which consecutive units go round the XCDs: a contiguous
 * range is spread evenly over all of them and their L2s.  Measured on MI355X (profiles/r04_notes.md): the effective granularity is 32
 * units (4 per XCD); the frame metrics on units [0, 64) beside the analysis + scan on [64, 256) take 8.2 ms per 10 000 frames instead
 * of 9.2 ms one after the other.  Use: one context per partition (amtgpu_context_set_stream), ordered against each other by the
 * caller's events.  NULL on failure (message on the context).  amtgpu_device_cu_count: compute units of the context's device. */
void*          amtgpu_stream_create_cu_range(AmtGpuContext* ctx, int first_cu, int num_cus);
void           amtgpu_stream_destroy(AmtGpuContext* ctx, void* hip_stream);
int            amtgpu_device_cu_count(AmtGpuContext* ctx);
/* per-kernel timing with HIP events on the launch stream (no counterpart in the reference, which only logs
 * phase wall times, CMAnalyze.hpp:37-39).  enable(1) resets the totals; report writes
 * "kernel_name calls total_ms\n" lines and returns the byte count (-1 on error). */
int            amtgpu_profile_enable(AmtGpuContext* ctx, int on);
int            amtgpu_profile_report(AmtGpuContext* ctx, char* out, int cap);

/* ---- frame ingest: pinned staging + hipMemcpyAsync on a side stream, double buffered against the
 *      compute stream (the step AMTSource::GetFrame feeds, AMTSource.hpp:721-780).  Allocates the device
 *      batch; free with amtgpu_device_free. ---- */
void* amtgpu_device_alloc(AmtGpuContext* ctx, uint64_t bytes);
void  amtgpu_device_free(AmtGpuContext* ctx, void* dptr);
int   amtgpu_frames_upload(AmtGpuContext* ctx, void* ddst, const void* hsrc, uint64_t bytes);   /* async on side stream */
/* the same for nchunks pieces of chunk_bytes that sit dst_stride apart on the device and src_stride apart on the host -- e.g. only
 * the logo rectangle's rows of every frame of a batch (h*pitch bytes instead of a whole frame: the logo passes read nothing
 * else).  async on the side stream */
int   amtgpu_frames_upload_strided(AmtGpuContext* ctx, void* ddst, int64_t dst_stride, const void* hsrc, int64_t src_stride,
                                   uint64_t chunk_bytes, int nchunks);
/* the same for `nsrc` separately allocated host frames at once: piece j of source i lands at ddst + (i * chunks_per_src + j) *
 * dst_stride -- one call and one copy launch for a whole group of PVideoFrames' logo rectangles (per-frame calls cost more in
 * API overhead than in bytes).  async on the side stream */
int   amtgpu_frames_upload_gather(AmtGpuContext* ctx, void* ddst, int64_t dst_stride, const void* const* hsrc, int64_t src_stride,
                                  uint64_t chunk_bytes, int chunks_per_src, int nsrc);
int   amtgpu_frames_upload_wait(AmtGpuContext* ctx);   /* make the compute stream wait for pending uploads */
/* Uploads from pageable host memory are staged through a ring of four pinned 32 MiB slots; the staging copy of a large upload is
 * shared out over `nthreads` threads (the caller's included; default min(4, cores / 4)) because one core's memcpy is below what
 * PCIe Gen5 x16 carries.  1 = the calling thread alone. */
int   amtgpu_context_set_upload_threads(AmtGpuContext* ctx, int nthreads);
/* Page-lock a host range in place (hipHostRegister) -- a decoder's frame pool, the buffers AMTSource keeps its frames in
 * (AMTSource.hpp:428-442): amtgpu_frames_upload / _upload_strided whose source lies inside a registered range skip the staging ring
 * and go out as one DMA copy straight from the caller's memory, which must stay untouched until amtgpu_frames_upload_wait's
 * consumer has run (or amtgpu_context_synchronize).  Registration costs about as much as touching every page once: register pools,
 * not frames.  unregister waits for the side stream first. */
int   amtgpu_frames_register(AmtGpuContext* ctx, void* hptr, uint64_t bytes);
int   amtgpu_frames_unregister(AmtGpuContext* ctx, void* hptr);
int   amtgpu_download(AmtGpuContext* ctx, void* hdst, const void* dsrc, uint64_t bytes);        /* synchronous */
/* nchunks pieces of chunk_bytes, src_stride apart on the device, dst_stride apart on the host (an erased rectangle back into
 * the rows of a host frame).  synchronous */
int   amtgpu_download_strided(AmtGpuContext* ctx, void* hdst, int64_t dst_stride, const void* dsrc, int64_t src_stride,
                              uint64_t chunk_bytes, int nchunks);
/* `bytes` from the device into a pinned landing buffer of the context: one asynchronous copy and one wait; *hptr is valid until
 * the next call.  For callers that scatter the bytes into several host frames themselves (a block of erased rectangles back into
 * the frames AMTEraseLogo::GetFrame serves, LogoScan.hpp:1343-1400). */
int   amtgpu_download_pinned(AmtGpuContext* ctx, const void* dsrc, uint64_t bytes, const void** hptr);
/* The same single copy, with the scatter done by the library while the context is still locked -- the form to use when several host
 * threads share one context (several filters of one script under Prefetch): piece i is nchunks runs of chunk_bytes that sit back to
 * back at dsrc + src_offset and go to hdst, dst_stride apart (an erased rectangle's rows back into the rows of a host frame). */
typedef struct AmtGpuScatter {
    void*    hdst;
    int64_t  dst_stride;
    uint64_t src_offset;
    uint64_t chunk_bytes;
    int      nchunks;
} AmtGpuScatter;
int   amtgpu_download_scatter(AmtGpuContext* ctx, const void* dsrc, uint64_t bytes, const AmtGpuScatter* pieces, int npieces);
/* Markers on the compute stream, ids 0..15: record(id) behind a batch's launches, wait(id) on the host before that batch's device
 * buffer is written again.  What a double-buffered caller (LogoFrame::scanFrames, LogoScan.hpp:1570-1589, over AMTSource::GetFrame)
 * needs instead of amtgpu_context_synchronize, which would also wait for the batch in flight.  wait on a never recorded id returns
 * at once. */
int   amtgpu_marker_record(AmtGpuContext* ctx, int id);
int   amtgpu_marker_wait(AmtGpuContext* ctx, int id);
/* The same pair on a marker the caller owns: users of a shared context (two LogoFrame scans, a filter next to user code) cannot
 * re-record each other's markers, whatever ids they would have picked. */
typedef struct AmtGpuMarker AmtGpuMarker;
AmtGpuMarker* amtgpu_marker_create(AmtGpuContext* ctx);
void  amtgpu_marker_destroy(AmtGpuContext* ctx, AmtGpuMarker* m);
int   amtgpu_marker_record_on(AmtGpuContext* ctx, AmtGpuMarker* m);
int   amtgpu_marker_wait_on(AmtGpuContext* ctx, AmtGpuMarker* m);     /* never recorded: returns at once */


/* ---- frame assembly: replaces AMTSource::MakeFrame -> MergeField / Copy1 / Copy2 (AMTSource.hpp:291-366) on decoded
 *      pictures already in HBM (uploaded with amtgpu_frames_upload): output frame i takes its even rows from picture
 *      top_index[i] and its odd rows from picture bottom_index[i] (the same picture for frame-coded streams, two for
 *      field-coded ones), plane by plane; nv12 != 0: the source chroma is ONE interleaved UV plane (dsrcU; dsrcV ignored)
 *      that is split into planar U and V (Copy2).  Pitches in ELEMENTS, strides in bytes; top_index / bottom_index are
 *      host arrays of nframes entries or NULL (= i).  The reference multiplies BYTE pitches into uint16_t pointers for
 *      > 8-bit pictures (:303-306 with T = uint16_t, :345-350); this uses element pitches, as every consumer of the frame
 *      does.  async unless index arrays are given ---- */
int   amtgpu_weave_fields_batch(AmtGpuContext* ctx, const void* dsrcY, const void* dsrcU, const void* dsrcV,
                                int64_t src_strideY, int64_t src_strideUV, int src_pitchY, int src_pitchUV, int num_pictures,
                                const int* top_index, const int* bottom_index, int nv12, int bits, int width, int height,
                                void* dY, void* dU, void* dV, int64_t strideY, int64_t strideUV, int pitchY, int pitchUV,
                                int nframes);

/* the same for MSB-aligned pictures (P010 / P012 decoder output: 16-bit containers with the sample in the high bits; bits 9..16 only):
 * every sample is read as container >> (16 - bits), whatever sits in the low bits is dropped, and the output is the usual planar LSB
 * clip.  Plane bases and strides must be multiples of 2.  This is the way into LogoFrame, AMTAnalyzeLogo and AMTEraseLogo for a P010 host */
int   amtgpu_weave_fields_batch_msb(AmtGpuContext* ctx, const void* dsrcY, const void* dsrcU, const void* dsrcV,
                                    int64_t src_strideY, int64_t src_strideUV, int src_pitchY, int src_pitchUV, int num_pictures,
                                    const int* top_index, const int* bottom_index, int nv12, int bits, int width, int height,
                                    void* dY, void* dU, void* dV, int64_t strideY, int64_t strideUV, int pitchY, int pitchUV,
                                    int nframes);

/* ---- decoder surfaces: what a hardware decoder or an FFmpeg hwframe hands out -- NV12 (8-bit Y plane plus one interleaved U0 V0 U1 V1 ...
 *      plane), P010 / P012 (the same layout in 16-bit containers with the sample in the HIGH bits) -- described once and taken as they are
 *      by every pass that reads frames in HBM: the ScanLogo session (amtgpu_scanlogo_stream_feed_surfaces, the logo
 *      rectangle), the logo finder (amtgpu_logofind_add_surfaces, the Y plane), the encode-time analysis and the LogoFrame scan
 *      (amtgpu_analyze_surfaces, amtgpu_logoframe_scan_surfaces: the logos' rows and columns of the Y plane), the erase
 *      (amtgpu_erase_surfaces...: the logo rectangle), the frame metrics (amtgpu_framestats_surfaces, _sharded_surfaces: the whole Y
 *      plane) and the cadence renderer (amtgpu_kfm_render: whole surfaces in, whole surfaces of the same kind out).  The sample rule is
 *      a plain right shift: whatever sits in the low 16 - bits bits
 *      of an MSB-aligned container is discarded (P010 says zero; decoders and dithering filters do not always leave zero there).
 *      The plane pointers are const because most entry points only read them; the ERASE entry points WRITE the planes the descriptor
 *      points to (amtgpu_erase_surfaces, amtgpu_erase_surfaces_dfades, and the dst of amtgpu_erase_surfaces_dfades_to), and
 *      amtgpu_kfm_render writes its dst: a COMPUTED MSB-aligned container is result << (16 - bits), its low bits zero, and a container
 *      that is only moved (a row the renderer copies, everything Delogo leaves alone) keeps its low bits.  4:2:0 only; linear (untiled,
 *      uncompressed) layouts only. ---- */
typedef struct AmtGpuSurfaces {
    const void* Y;               /* luma plane of the first picture (device) */
    const void* U;               /* planar: U plane.  interleaved: the UV plane (U0 V0 U1 V1 ...) */
    const void* V;               /* planar: V plane.  interleaved: ignored, may be NULL */
    int64_t strideY, strideUV;   /* bytes between pictures (Y and UV of one allocation: both = the surface size) */
    int pitchY, pitchUV;         /* container elements per row; of the UV plane when interleaved (>= 2 * chroma width) */
    int bits;                    /* 8 (uint8 containers) or 9..16 (little-endian uint16 containers) */
    int interleaved;             /* 0 planar, 1 NV12 / P010 layout */
    int msb_aligned;             /* 0: sample = container.  1: sample = container >> (16 - bits); refused at bits == 8 */
    int reserved;                /* 0 */
} AmtGpuSurfaces;
/* the rectangle (imgx, imgy, w, h) of nframes surfaces as planar LSB samples of depth src->bits: w x h luma at dY, w/2 x h/2 chroma
 * (origin imgx >> 1, imgy >> 1) at dU / dV per frame, frames dstrideY / dstrideUV BYTES apart, rows dpitchY / dpitchUV SAMPLES -- what
 * amtgpu_scanlogo_stream_feed_rect and amtgpu_erase_rect_batch take.  w, h even and positive, the rectangle inside the pitches;
 * (0, 0, W, H) planarises whole progressive frames.  Reads nothing outside the rectangle's rows, writes nothing outside w / w/2 samples
 * of a destination row.  nframes == 0 returns 1.  async */
int   amtgpu_surfaces_extract_rect(AmtGpuContext* ctx, const AmtGpuSurfaces* src, int imgx, int imgy, int w, int h, int nframes,
                                   void* dY, void* dU, void* dV, int64_t dstrideY, int64_t dstrideUV, int dpitchY, int dpitchUV);

/* ---- the stream-index file AMTSource is built from: replaces LoadAMTSource's reader (AMTSource.hpp:854-871; writer :835-852,
 *      File::writeArray framing CoreUtils.hpp:275-284, FilterSourceFrame StreamReform.hpp:145-154) and the frame-assembly rule of
 *      AMTSource::OnFrameOutput (:482-566).  MSVC x64 POD layouts with 2-byte wchar_t, parsed with fixed offsets. ---- */
typedef struct AmtGpuAmtsFile AmtGpuAmtsFile;
AmtGpuAmtsFile* amtgpu_amts_load(AmtGpuContext* ctx, const char* path);      /* ctx may be NULL (no message kept then) */
void amtgpu_amts_destroy(AmtGpuAmtsFile* a);
/* out19 = VideoFormat {format, width, height, displayWidth, displayHeight, sarWidth, sarHeight, frameRateNum, frameRateDenom,
 * colorPrimaries, transferCharacteristics, colorSpace, progressive, fixedFrameRate}, AudioFormat {channels, sampleRate},
 * DecoderSetting {mpeg2, h264, hevc} */
int  amtgpu_amts_get_info(const AmtGpuAmtsFile* a, int* out19, int* num_frames, int* num_audio_frames);
/* source TS path and audio wave path, UTF-16 converted to UTF-8; 0 if a buffer is too small */
int  amtgpu_amts_get_paths(const AmtGpuAmtsFile* a, char* srcpath, int cap_src, char* audiopath, int cap_audio);
/* per-frame columns of the FilterSourceFrame list (num_frames entries each; any pointer may be NULL) */
int  amtgpu_amts_get_frames(const AmtGpuAmtsFile* a, int64_t* framePTS, int64_t* fileOffset, int* keyFrame, uint8_t* halfDelay, int* cmType);
/* Which decoded pictures make which frame: picture_pts = PTS of the decoded pictures in output order.  For frame i the top field
 * comes from picture top_index[i] and the bottom field from bottom_index[i] (both -1: the frame cannot be made from this sequence,
 * e.g. a half-delayed frame right after a discontinuity) -- the arrays amtgpu_weave_fields_batch takes. */
int  amtgpu_amts_weave_plan(const AmtGpuAmtsFile* a, const int64_t* picture_pts, int npictures, int* top_index, int* bottom_index);
/* The clip's audio timeline as AMTSource presents it (MakeVideoInfo, AMTSource.hpp:239-250): 16-bit stereo sample-frames of 4 bytes,
 * samples_per_frame = 1024, replaced by waveLength / 4 of the first audio frame whose waveLength != 0, and
 * num_samples = samples_per_frame * num_audio_frames.  Both are 0 for a clip without audio frames. */
int  amtgpu_amts_audio_info(const AmtGpuAmtsFile* a, int* samples_per_frame, int64_t* num_samples);
/* columns of the FilterAudioFrame list (num_audio_frames entries each; any pointer may be NULL) */
int  amtgpu_amts_get_audio_frames(const AmtGpuAmtsFile* a, int* frameIndex, int64_t* waveOffset, int* waveLength);
/* AMTSource::GetAudio (AMTSource.hpp:782-817): `count` sample-frames from `start` on into out (count * 4 bytes: 16-bit stereo, whatever
 * AudioFormat.channels says).  Audio frame k supplies sample-frames [k spf, (k + 1) spf) from waveOffset on -- spf * 4 bytes, not limited
 * by its waveLength -- or zeros when its waveLength is 0; everything behind the last audio frame is zero.  wavepath NULL: the file's own
 * audiopath.  Audio frames that follow each other in the wave file are read with one read.  0, with a message on the context the file
 * was loaded with: negative start or count, a clip without audio frames, a file that cannot be opened, a short read.  count == 0
 * returns 1 and touches neither `out` nor the wave file. */
int  amtgpu_amts_read_audio(const AmtGpuAmtsFile* a, const char* wavepath, int64_t start, int64_t count, int16_t* out);

/* ---- logo model: replaces LogoData::Load / Save (AMTLogo.hpp:239-279), LogoFile_* getters
 *      (LogoGUISupport.hpp:254-275) ---- */
AmtGpuLogo* amtgpu_logo_load(AmtGpuContext* ctx, const char* path);
/* paths as the reference's exports take them: NUL-terminated UTF-16 (const tchar* = wchar_t* on Windows, LogoScan.hpp:1083-1086;
 * C# CharSet.Unicode, AmatsukazeNatives.cs:391-393).  Converted to UTF-8 for the file system here (Linux). */
AmtGpuLogo* amtgpu_logo_loadW(AmtGpuContext* ctx, const uint16_t* path);
/* planes = aY,bY,aU,bU,aV,bV back to back (AMTLogo.hpp:204-212) */
AmtGpuLogo* amtgpu_logo_from_planes(AmtGpuContext* ctx, int w, int h, int logUVx, int logUVy,
                                    int imgw, int imgh, int imgx, int imgy, const float* planes);
int  amtgpu_logo_save(AmtGpuContext* ctx, const AmtGpuLogo* logo, const char* path, const char* name, int serviceId);
int  amtgpu_logo_saveW(AmtGpuContext* ctx, const AmtGpuLogo* logo, const uint16_t* path, const char* name, int serviceId);
/* LogoFile_GetName / GetServiceId / SetName / SetServiceId (LogoGUISupport.hpp:254-275) of the extended header (AMTLogo.hpp:19-47):
 * name is UTF-8 bytes as stored (at most 254 + NUL); either out pointer of get may be NULL */
int  amtgpu_logo_get_header(const AmtGpuLogo* logo, char* name, int name_cap, int* serviceId);
int  amtgpu_logo_set_header(AmtGpuLogo* logo, const char* name, int serviceId);
void amtgpu_logo_destroy(AmtGpuLogo* logo);
/* out[8] = w,h,logUVx,logUVy,imgw,imgh,imgx,imgy */
int  amtgpu_logo_get_info(const AmtGpuLogo* logo, int* out8);
int  amtgpu_logo_get_planes(const AmtGpuLogo* logo, float* out);
/* evaluation tables of LogoDataParam::CreateLogoMask (LogoScan.hpp:112-229) for inspection / tests:
 * kind 0 = DeintLogo'ed logo, 1 = top-field logo, 2 = bottom-field logo (MakeFieldLogo :257-283).
 * Any out pointer may be NULL.  mask: w*h bytes; kernels: count*25; scales: count*32*{scale,scale2}. */
int  amtgpu_logo_mask_tables(AmtGpuContext* ctx, const AmtGpuLogo* logo, int kind, float maskratio,
                             int* maskpixels, int* count, float* blackScore,
                             uint8_t* mask, float* kernels, float* scales);

/* ---- CM all-frames logo scan: replaces logo::LogoFrame (ctor :1592-1616, scanFrames :1618-1630,
 *      selectLogo :1647-1682, writeResult :1686-1827, getBestLogo/getLogoRatio :1829-1835) as driven by
 *      CMAnalyze::logoFrame (CMAnalyze.hpp:273-317).  Unreadable logo files are ignored like the
 *      reference does (:1612-1614) and score {0,-1}. ---- */
AmtGpuLogoFrame* amtgpu_logoframe_create(AmtGpuContext* ctx, const char* const* logopaths, int nlogos, float maskratio);
AmtGpuLogoFrame* amtgpu_logoframe_create_from_logos(AmtGpuContext* ctx, const AmtGpuLogo* const* logos, int nlogos, float maskratio);
void amtgpu_logoframe_destroy(AmtGpuLogoFrame* lf);
/* declare the clip (VideoInfo): resets results to num_frames entries */
int  amtgpu_logoframe_begin(AmtGpuLogoFrame* lf, int width, int height, int bits, int num_frames, int fps_num, int fps_den);
/* scan frames [first, first+nframes) of the clip from a device batch (Y plane only).  async */
int  amtgpu_logoframe_scan_batch(AmtGpuLogoFrame* lf, const void* dY, int64_t frame_stride, int pitch, int first, int nframes);
/* amtgpu_logoframe_scan_batch on the Y planes of a batch of surfaces; batch->bits must be the depth given to amtgpu_logoframe_begin.  async
 * LSB surfaces are read where they lie.  Of MSB-aligned surfaces the band the scan reads (amtgpu_logoframe_get_rows x _get_columns of the
 * logos that match the clip) is first copied as LSB samples into a scratch buffer the object owns (it grows to the largest batch seen):
 * the surfaces entry point of one object is therefore NOT re-entrant.  nframes == 0 returns 1 */
int  amtgpu_logoframe_scan_surfaces(AmtGpuLogoFrame* lf, const AmtGpuSurfaces* batch, int first, int nframes);
/* results: num_frames*nlogos*{corr0,corr1} (EvalResult, LogoScan.hpp:1532-1535) */
/* out2 = {first row, one past the last row} of the Y plane that the scan of these logos reads (the union of their rectangles) */
int  amtgpu_logoframe_get_rows(const AmtGpuLogoFrame* lf, int* out2);
/* ... and {first column, one past the last column}: a caller that ships frames over PCIe needs to bring no other samples */
int  amtgpu_logoframe_get_columns(const AmtGpuLogoFrame* lf, int* out2);
int  amtgpu_logoframe_get_results(AmtGpuLogoFrame* lf, float* out);
/* sharded scans: install results computed elsewhere (other ranks) for frames [first, first+nframes) */
int  amtgpu_logoframe_set_results(AmtGpuLogoFrame* lf, int first, int nframes, const float* evals);
int  amtgpu_logoframe_select_logo(AmtGpuLogoFrame* lf, int num_candidates);        /* -1 = all */
int  amtgpu_logoframe_write_result(AmtGpuLogoFrame* lf, const char* outpath, int logo_index); /* -1 = best */
/* LogoFrame::dumpResult (LogoScan.hpp:1632-1643): one text file per logo, "<basepath><logo index>", a line "%f,%f\n" {corr0, corr1} per frame */
int  amtgpu_logoframe_dump_result(AmtGpuLogoFrame* lf, const char* basepath);
int  amtgpu_logoframe_best_logo(const AmtGpuLogoFrame* lf);
/* The same two decisions -- LogoFrame::selectLogo and the text LogoFrame::writeResult writes (LogoScan.hpp:1647-1827) -- from scan
 * records alone, on the host, no device and no LogoFrame object: what a rank (or a tool) that only holds the gathered
 * records [num_frames][num_logos]{corr0, corr1} needs.  logo_index -1 = the selected logo.  text may be NULL (cap 0) to ask for
 * the length.  Returns 1 = done, 0 = failed: bad arguments (NULL records, logo_index or num_candidates > num_logos, fps <= 0) or cap
 * too small -- then *text_len (set whenever the arguments are good) is > cap and says how much it takes.  O(1) work per frame.  Evidence that is NaN (corr0 = +inf with corr1 = -inf) sorts after
 * every number in the median window -- the reference's std::sort over it is undefined. */
int  amtgpu_logoframe_decide_host(const float* evals, int num_frames, int num_logos, int num_candidates, int logo_index,
                                  int fps_num, int fps_den, int* best_logo, float* logo_ratio, char* text, int cap, int* text_len);
float amtgpu_logoframe_logo_ratio(const AmtGpuLogoFrame* lf);

/* ---- encode-time analysis: replaces logo::AMTAnalyzeLogo ("AMTAnalyzeLogo" "cs[maskratio]i",
 *      Amatsukaze.cpp:58; ctor :1164-1201, GetFrameT :1119-1161).  One record of 33 floats
 *      {p[11],t[11],b[11]} per SOURCE frame; the AviSynth shim packs 8 per BGR32 frame (:1195-1200). ---- */
AmtGpuAnalyze* amtgpu_analyze_create(AmtGpuContext* ctx, const char* logopath, float maskratio);
AmtGpuAnalyze* amtgpu_analyze_create_from_logo(AmtGpuContext* ctx, const AmtGpuLogo* logo, float maskratio);
void amtgpu_analyze_destroy(AmtGpuAnalyze* an);
/* dout: device buffer of nframes*33 floats.  async */
int  amtgpu_analyze_batch(AmtGpuAnalyze* an, const void* dY, int64_t frame_stride, int pitch, int bits, int nframes, float* dout);
/* amtgpu_analyze_batch on the Y planes of a batch of surfaces (depth = batch->bits); dout: nframes*33 floats on the device.  async
 * LSB surfaces are read where they lie.  Of MSB-aligned surfaces the rectangle's rows (columns from imgx rounded down to 64 containers)
 * are first copied as LSB samples into a scratch buffer the object owns (it grows to the largest batch seen): the surfaces entry point of
 * one object is therefore NOT re-entrant.  nframes == 0 returns 1 */
int  amtgpu_analyze_surfaces(AmtGpuAnalyze* an, const AmtGpuSurfaces* batch, int nframes, float* dout);
/* convenience: same, results copied to host (synchronises) */
/* out4 = {imgx, imgy, w, h}: the rectangle the analysis reads (LogoScan.hpp:1132-1141) -- a host that uploads frames may ship only
 * the rows [imgy, imgy+h) of every Y plane, at their place in the frame: nothing else is read */
int  amtgpu_analyze_get_rect(const AmtGpuAnalyze* an, int* out4);
int  amtgpu_analyze_batch_host(AmtGpuAnalyze* an, const void* dY, int64_t frame_stride, int pitch, int bits, int nframes, float* hout);

/* Evaluation mode of the 33 scores per frame.
 *   AMTGPU_ANALYZE_EXACT (default): every fade evaluated in the reference's fp32 order -- records are bit-identical to
 *     AMTAnalyzeLogo::GetFrameT's.
 *   AMTGPU_ANALYZE_LINEAR_GUARDED: CalcCorrelation5x5 is linear in the window (ComputeKernel.cpp:77-121), so the 11 blends are
 *     formed from ONE evaluation of the source window and ONE of the background-estimate window per mask pixel (~4x less
 *     arithmetic).  Scores differ from the reference's by rounding only (|diff| <= amtgpu_analyze_error_bound, typically 1e-6;
 *     the north star allows 1e-4), and the integer decisions taken from them are guarded: bins are selected from the exactly
 *     evaluated mean whenever the interpolated one is near a bin edge, and every frame whose argmin over the fades of p, t or b
 *     (all CalcFade2 ever reads, LogoScan.hpp:1288-1314) is not separated by more than twice the error bound is re-evaluated by
 *     the exact kernel before the batch is handed out -- amtgpu_erase_calc_fades returns identical fades in both modes. */
#define AMTGPU_ANALYZE_EXACT 0
#define AMTGPU_ANALYZE_LINEAR_GUARDED 1
#define AMTGPU_ANALYZE_LINEAR_UNGUARDED 2   /* the linear evaluation alone, without the argmin guard: for accuracy tests and profiling */
/*   AMTGPU_ANALYZE_LINEAR_MONITORED: the guarded linear mode, and in every batch K sentinel frames are evaluated exactly as well (frames
 *     floor(j (nframes - 1) / (K' - 1)), j < K' = min(K, nframes); K' = 1: frame 0 -- the first and the last frame of a batch whenever
 *     K' > 1).  Their 33 linear scores are compared with the exact ones on the device; a score with !(|linear - exact| <= tolerance) trips
 *     the monitor (NaN against a number trips, NaN against NaN is equal; frames with samples above maxv are exact anyway and not compared).
 *     A batch that passes hands out the exact records on the sentinels and mode 1's everywhere else; a batch that trips is re-evaluated
 *     exactly in the same stream (records = the exact mode's), and the analyzer stays exact from then on ("downgraded") until
 *     amtgpu_analyze_set_mode(an, AMTGPU_ANALYZE_LINEAR_MONITORED) re-arms it.  The monitor SAMPLES: it vouches for every compared frame
 *     and, once a comparison has failed, for every later record; it proves nothing about frames it did not compare.  async like mode 1. */
#define AMTGPU_ANALYZE_LINEAR_MONITORED 3
/* (setting AMTGPU_ANALYZE_LINEAR_MONITORED, also when it is already set, re-arms the monitor: no downgrade, statistics zeroed) */
int   amtgpu_analyze_set_mode(AmtGpuAnalyze* an, int mode);
/* the monitor's absolute tolerance on the normalised scores (finite, >= 0; 0: any difference trips; default 1e-4) and sentinels per batch
 * (>= 1; default 16); valid in any mode, used from the next monitored batch on */
int   amtgpu_analyze_set_monitor(AmtGpuAnalyze* an, float tolerance, int sentinels);
/* since the monitor was last armed: the largest |linear - exact| of a compared score (+inf for NaN against a number), sentinel frames
 * compared, whether it has downgraded.  Synchronises; any pointer may be null */
int   amtgpu_analyze_monitor_stats(AmtGpuAnalyze* an, float* max_abs, int64_t* frames_checked, int* downgraded);
/* frames of the most recent batch that the guard re-evaluated exactly (synchronises); 0 in exact mode, -1 on error.  Monitored mode: the
 * frames whose records came from the exact kernel -- the guard's and the sentinels, or all of a batch that tripped or ran downgraded */
int   amtgpu_analyze_last_refined(AmtGpuAnalyze* an);
/* Linear modes: (pixel, frame, fade) pairs whose window mean lies within the evaluation's error bound of a bin edge (LogoScan.hpp:304 is
 * discontinuous there) are listed per wave and settled exactly when the workgroup has finished; a workgroup whose list overflows leaves
 * its frames to the exact kernel (they are counted by amtgpu_analyze_last_refined).  entries = pairs a wave can list, 16 .. 640,
 * default 256; fewer frames share a workgroup as the list grows (LDS).  A tuning knob: results do not depend on it. */
int   amtgpu_analyze_set_fixup_queue(AmtGpuAnalyze* an, int entries);
/* the linear mode's bound on |score - reference score| for group 0 = p, 1 = t, 2 = b at the given bit depth; 0 in exact mode and in a
 * downgraded monitored mode (which synchronises to find out) */
float amtgpu_analyze_error_bound(AmtGpuAnalyze* an, int group, int bits);

/* ---- encode-time erase: replaces logo::AMTEraseLogo ("AMTEraseLogo" "ccs[logof]s[mode]i[maxfade]i",
 *      Amatsukaze.cpp:59; ctor :1464-1481, ReadLogoFrameFile :1421-1461, CalcFade :1317-1341,
 *      CalcFade2 :1263-1315, Delogo :1248-1261, GetFrameT mode 0 :1343-1400).  logofpath may be "" ---- */
AmtGpuErase* amtgpu_erase_create(AmtGpuContext* ctx, const char* logopath, const char* logofpath, int mode, int maxfade);
AmtGpuErase* amtgpu_erase_create_from_logo(AmtGpuContext* ctx, const AmtGpuLogo* logo, const char* logof_text, int mode, int maxfade);
void amtgpu_erase_destroy(AmtGpuErase* er);
/* fades for frames [first, first+nframes) of a num_frames clip from the per-source-frame analysis of the
 * WHOLE clip (host, num_frames*33 floats).  out = nframes*{fadeT,fadeB}.  Host-only (tiny). */
int  amtgpu_erase_calc_fades(AmtGpuErase* er, const float* analysis, int num_frames, int first, int nframes, float* fades_out);
/* in-place erase of a device batch with the given per-frame fades (host array nframes*2).  async */
int  amtgpu_erase_batch(AmtGpuErase* er, void* dY, void* dU, void* dV, int64_t strideY, int64_t strideUV,
                        int pitchY, int pitchUV, int bits, int nframes, const float* fades);
/* the same on planes that hold ONLY the logo rectangle (w x h luma, w/2 x h/2 chroma samples per frame, first sample = the
 * rectangle's top-left): what a per-frame host filter ships instead of whole frames -- Delogo touches nothing else
 * (LogoScan.hpp:1248-1261, 1374-1397).  async */
int  amtgpu_erase_rect_batch(AmtGpuErase* er, void* dY, void* dU, void* dV, int64_t strideY, int64_t strideUV,
                             int pitchY, int pitchUV, int bits, int nframes, const float* fades);
/* CalcFade / CalcFade2 (LogoScan.hpp:1263-1341) on the DEVICE: the same decision as amtgpu_erase_calc_fades, frame by frame in one small
 * kernel, from analysis records that are still in HBM (the output of amtgpu_analyze_batch) -- no host round trip between analysis
 * and erase, the whole analyse -> decide -> erase chain is stream-ordered.  d_analysis holds the records of source frames
 * [analysis_first, analysis_first + analysis_count) of a num_frames clip, 33 floats each; it must cover every record the fades of
 * [first, first + nframes) read: frames max(0, first - 8) .. min(num_frames, first + nframes + 8) - 1 (CalcFade2 samples n - 8 .. n + 8;
 * near the clip ends the reference's clamped indices stay inside that range).  d_fades_out: nframes * {fadeT, fadeB} floats on the
 * device, bit-identical to the host routine's.  async */
int  amtgpu_erase_calc_fades_device(AmtGpuErase* er, const float* d_analysis, int analysis_first, int analysis_count, int num_frames,
                                    int first, int nframes, float* d_fades_out);
/* amtgpu_erase_batch / amtgpu_erase_rect_batch with the fades taken from DEVICE memory (nframes * 2 floats, e.g. the output of
 * amtgpu_erase_calc_fades_device).  async */
int  amtgpu_erase_batch_dfades(AmtGpuErase* er, void* dY, void* dU, void* dV, int64_t strideY, int64_t strideUV,
                               int pitchY, int pitchUV, int bits, int nframes, const float* d_fades);
int  amtgpu_erase_rect_batch_dfades(AmtGpuErase* er, void* dY, void* dU, void* dV, int64_t strideY, int64_t strideUV,
                                    int pitchY, int pitchUV, int bits, int nframes, const float* d_fades);
/* amtgpu_erase_batch_dfades from a SOURCE batch into a DESTINATION batch of the same geometry (strides, pitches, bit depth) that already
 * holds a copy of the source frames -- the writable copy AMTEraseLogo::GetFrameT takes before it calls Delogo (env->MakeWritable,
 * LogoScan.hpp:1346-1347): Delogo reads the source's rectangle and writes the destination's.  The source stays intact for its other
 * consumers (the frame metrics, the scan, the next pass over the same frames); what Delogo leaves alone -- every sample outside the
 * rectangle, frames whose fades are {0, 0} (see amtgpu_erase_get_rect), an odd last chroma row in field mode -- is NOT written, it is
 * the copy's.  sY == dY (all three) is amtgpu_erase_batch_dfades.  async (ABI 5) */
int  amtgpu_erase_batch_dfades_to(AmtGpuErase* er, const void* sY, const void* sU, const void* sV, void* dY, void* dU, void* dV,
                                  int64_t strideY, int64_t strideUV, int pitchY, int pitchUV, int bits, int nframes, const float* d_fades);
/* Delogo in place on a batch of decoder surfaces; fades: host array nframes*2 / device array.  The planes the descriptor points to ARE WRITTEN.  async
 * Rewritten: the containers of the logo rectangle (interleaved chroma: containers 2*cx .. 2*(cx + w/2) - 1 of its rows), as
 * msb_aligned ? result << (16 - bits) : result.  Not rewritten means not touched, low bits included: everything outside the rectangle, an
 * odd last chroma row in field mode, and frames whose fades are {0, 0} when fade0_is_identity (amtgpu_erase_get_rect) holds and bits is
 * 8 or 16 or the surfaces are MSB-aligned (an MSB sample never exceeds maxv; LSB 9..15-bit containers are computed, as in
 * amtgpu_erase_batch).  Refused: a null descriptor, reserved != 0, bad bits, a pitch smaller than the rectangle's rows, mode != 0, null
 * fades.  nframes == 0 returns 1 and touches nothing */
int  amtgpu_erase_surfaces(AmtGpuErase* er, const AmtGpuSurfaces* batch, int nframes, const float* fades);
int  amtgpu_erase_surfaces_dfades(AmtGpuErase* er, const AmtGpuSurfaces* batch, int nframes, const float* d_fades);
/* reads src, writes dst, which already holds a copy of the pictures (MakeWritable semantics of amtgpu_erase_batch_dfades_to); dst must equal src in
 * bits, interleaved, msb_aligned, pitches and strides; src == dst (same planes) is the in-place call */
int  amtgpu_erase_surfaces_dfades_to(AmtGpuErase* er, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes, const float* d_fades);
/* out5 = {imgx, imgy, w, h, fade0_is_identity}: the rectangle Delogo rewrites; the last word is 1 when a frame whose two fades
 * are 0 comes back unchanged (every a*s + b*maxv of this logo is finite), i.e. the host may skip the call for such frames --
 * of an 8- or 16-bit clip: at 10 / 12 bits Delogo's min(tmp + 0.5, maxv) (LogoScan.hpp:1258) still clamps container values
 * above maxv, so those frames must go through (the library itself skips fade-0 frames only at 8 and 16 bits) */
int  amtgpu_erase_get_rect(const AmtGpuErase* er, int* out5);

/* ---- logo generation: replaces logo::LogoScan (AddFrame :594-659, AddScanFrame :568-592,
 *      Normalize :471-488, GetLogo :490-566) and LogoAnalyzer / the exported ScanLogo (:794-1098) ---- */
AmtGpuLogoScan* amtgpu_logoscan_create(AmtGpuContext* ctx, int w, int h, int logUVx, int logUVy, int thy);
void amtgpu_logoscan_destroy(AmtGpuLogoScan* s);
/* planes of full frames; the scan rectangle sits at (imgx,imgy).  valid_out (host, nframes bytes, may be
 * NULL) receives AddFrame's verdict per frame.  At most `max_valid` further frames are accepted, in
 * stream order (numMaxFrames, :885).  Returns 1/0; *naccepted = frames accepted by this call.
 * use_mask (host, nframes bytes, may be NULL): only frames with use_mask[i]!=0 are offered (ReMakeLogo :1018) */
int  amtgpu_logoscan_add_batch(AmtGpuLogoScan* s, const void* dY, const void* dU, const void* dV,
                               int64_t strideY, int64_t strideUV, int pitchY, int pitchUV, int bits,
                               int imgx, int imgy, int nframes, int max_valid, const uint8_t* use_mask,
                               uint8_t* valid_out, int* naccepted);
int  amtgpu_logoscan_nframes(const AmtGpuLogoScan* s);
/* exact integer sums per pixel {sumF, sumF2, sumFB} (Y then U then V) + per plane {sumB, sumB2}: for the
 * sharded all-reduce.  sums: 3*(w*h+2*wUV*hUV) int64; plane_sums: 6 int64. */
int  amtgpu_logoscan_get_sums(AmtGpuLogoScan* s, int64_t* sums, int64_t* plane_sums);
int  amtgpu_logoscan_set_sums(AmtGpuLogoScan* s, const int64_t* sums, const int64_t* plane_sums, int nframes);
/* Normalize(maxv) + GetLogo(clean); NULL (+ error) when the regression fails ("Insufficient logo frames") */
AmtGpuLogo* amtgpu_logoscan_get_logo(AmtGpuLogoScan* s, int maxv, int clean, int imgw, int imgh, int imgx, int imgy);
/* Same signature family as the reference's ScanLogo (LogoScan.hpp:1083-1098), over a device-resident
 * 8-bit clip instead of a TS path: 1 ok / 0 fail. */
int  amtgpu_scanlogo(AmtGpuContext* ctx, const void* dY, const void* dU, const void* dV,
                     int64_t strideY, int64_t strideUV, int pitchY, int pitchUV, int imgw, int imgh,
                     int nframes, int serviceid, const char* dstpath, int imgx, int imgy, int w, int h,
                     int thy, int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb);
/* The same for a clip `bits` deep.  8: amtgpu_scanlogo itself, identical bytes.  9..12: uint16 little-endian containers (strides in
 * bytes, pitches in elements), ScanLogo (:917-1079) stated with pixel_t = uint16_t and maxv = (1 << bits) - 1 wherever the 8-bit path
 * writes 255 (Normalize, EvaluateLogo, DeintY), as AMTAnalyzeLogo (:1130) and AMTEraseLogo (:1349) state it; an extension the
 * reference cannot pin beyond its template text (its scan is 8-bit because of its work-file codec, :813).  DESIGN.md section 9.
 * thy is compared unscaled, in container units: a GUI's 12 at 8 bits is 48 at 10 bits.  The .lgd is depth-agnostic (coefficients
 * normalised by maxv).  Refused with a message: bits outside 8..12, thy >= 1 << bits when bits > 8, an odd byte stride or a plane
 * base that is not a multiple of 2 when bits > 8.  The _bits variants below follow the same rules. */
int  amtgpu_scanlogo_bits(AmtGpuContext* ctx, const void* dY, const void* dU, const void* dV,
                          int64_t strideY, int64_t strideUV, int pitchY, int pitchUV, int imgw, int imgh, int bits,
                          int nframes, int serviceid, const char* dstpath, int imgx, int imgy, int w, int h,
                          int thy, int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb);

/* The reference's exported ScanLogo with its own argument list (LogoScan.hpp:1083-1098; AmatsukazeNatives.cs:391-393):
 * (ctx, srcpath, serviceid, workfile, dstpath, imgx, imgy, w, h, thy, numMaxFrames, cb) -> 1 ok / 0 fail + amtgpu_last_error.
 * srcpath is a raw 8-bit 4:2:0 clip (int32 'AMTR', width, height, frames, then tight Y,U,V per frame) instead of a transport stream
 * (demux / decode are out of scope), or a raw 9..12-bit one: little-endian int32 {'AMTH' = 0x48544D41, width, height, frames, bits}, then
 * tight Y,U,V per frame as little-endian uint16 (the depth comes from the file; bits 8 or above 12 in an 'AMTH' header is refused).
 * Frames stream through the pinned ring, accepted rectangles stay in HBM; workfile is unused. */
int  amtgpu_scanlogo_file(AmtGpuContext* ctx, const char* srcpath, int serviceid, const char* workfile, const char* dstpath,
                          int imgx, int imgy, int w, int h, int thy, int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb);
/* the same with the reference's string type: NUL-terminated UTF-16 paths (P/Invoke CharSet.Unicode keeps working) */
int  amtgpu_scanlogo_fileW(AmtGpuContext* ctx, const uint16_t* srcpath, int serviceid, const uint16_t* workfile, const uint16_t* dstpath,
                           int imgx, int imgy, int w, int h, int thy, int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb);

/* ---- ScanLogo as a streaming session: the same logo generation for a host that decodes (an FFmpeg loop, an AviSynth clip, a pipe)
 *      and cannot hold the clip in HBM.  create with the rectangle, feed device batches in stream order as they arrive, finish to get
 *      the .lgd -- byte-identical to amtgpu_scanlogo over the same frames.  4:2:0; 8-bit like the reference's ScanLogo (LogoScan.hpp:813),
 *      or 9..12-bit through amtgpu_scanlogo_stream_create_bits.  What
 *      the session keeps in HBM is the rectangle of every kept frame (w*h*3/2 samples each; the reference's work file, :899-903): the
 *      store starts at min(numMaxFrames, 256) frames and doubles, so numMaxFrames may be "no limit" (1 << 30).
 *      amtgpu_scanlogo_file is a client of it. ---- */
typedef struct AmtGpuScanLogoStream AmtGpuScanLogoStream;
/* NULL (message on the context) for the rectangles amtgpu_scanlogo refuses: outside the imgw x imgh frame, odd or non-positive w / h.
 * numMaxFrames < 0 counts as 0 */
AmtGpuScanLogoStream* amtgpu_scanlogo_stream_create(AmtGpuContext* ctx, int imgw, int imgh, int imgx, int imgy, int w, int h,
                                                    int thy, int numMaxFrames);
/* the same for frames `bits` deep (8..12, as amtgpu_scanlogo_bits; a bad depth or thy >= 1 << bits above 8 bits is refused here).  The
 * session knows its depth: feed, feed_rect, status and both finishes are the ones below, with uint16 planes when bits > 8 */
AmtGpuScanLogoStream* amtgpu_scanlogo_stream_create_bits(AmtGpuContext* ctx, int imgw, int imgh, int bits, int imgx, int imgy, int w, int h,
                                                         int thy, int numMaxFrames);
void amtgpu_scanlogo_stream_destroy(AmtGpuScanLogoStream* s);
/* the next nframes frames of the stream, full frames on the device (strides in bytes, pitches in elements).  Valid frames (AddFrame's
 * border verdict, :604-653) are kept in stream order until numMaxFrames are kept (:885); the frame that fills the quota may sit in
 * the middle of a batch -- the frames behind it are neither kept nor counted as read.  *nkept = frames kept so far, *done = 1 from the
 * call that fills the quota on (either may be NULL); a feed after that, or of 0 frames, returns 1 and changes nothing.
 * Returns once the batch's verdicts have been read back (synchronises the context's stream up to them); the copy of the kept
 * rectangles is only ENQUEUED on that stream when the call returns: overwrite the batch with work on the same stream, or after a
 * marker / amtgpu_context_synchronize from anywhere else. */
int  amtgpu_scanlogo_stream_feed(AmtGpuScanLogoStream* s, const void* dY, const void* dU, const void* dV, int64_t strideY, int64_t strideUV,
                                 int pitchY, int pitchUV, int nframes, int* nkept, int* done);
/* the same on planes that hold ONLY the rectangle (w x h luma, w/2 x h/2 chroma per frame), as amtgpu_erase_rect_batch takes them */
int  amtgpu_scanlogo_stream_feed_rect(AmtGpuScanLogoStream* s, const void* dY, const void* dU, const void* dV, int64_t strideY, int64_t strideUV,
                                      int pitchY, int pitchUV, int nframes, int* nkept, int* done);
/* the same on decoder surfaces (AmtGpuSurfaces above: NV12, P010, planar MSB ...; batch->bits must be the session's depth): the session's
 * rectangle of all nframes surfaces goes to a scratch buffer the session owns (it grows to the largest batch seen) as planar LSB planes,
 * then feed_rect's path runs on it -- the same verdicts, quota and store.  Only the rectangle is read: ~1/30 of the bytes a planarising
 * weave of whole 1440 x 1080 frames moves for a 256 x 128 logo.  feed, feed_rect and feed_surfaces may be mixed within one session; the
 * batch may be overwritten as after feed */
int  amtgpu_scanlogo_stream_feed_surfaces(AmtGpuScanLogoStream* s, const AmtGpuSurfaces* batch, int nframes, int* nkept, int* done);
/* *nread = the reference's readCount (:883): frames consumed up to and including the one that closed the stream; any pointer may be NULL */
int  amtgpu_scanlogo_stream_status(const AmtGpuScanLogoStream* s, int64_t* nread, int* nkept, int* done);
/* the initial regression and the two ReMakeLogo rounds (:923-1036) over the kept rectangles, cb driven from 50 % upward as by
 * amtgpu_scanlogo; writes dstpath.  0 with "Insufficient logo frames" when nothing was kept or the regression fails, 0 with "Cancel
 * requested" when cb returns 0.  The session is spent afterwards, whatever the outcome: a later feed or finish returns 0 with a message;
 * destroy is always allowed. */
int  amtgpu_scanlogo_stream_finish(AmtGpuScanLogoStream* s, int serviceid, const char* dstpath, AMTGPU_LOGO_ANALYZE_CB cb);

/* ---- frame-sharded runs (one process per GPU).  The library does no communication itself: the host
 *      supplies two collectives over HOST memory -- RCCL in a C++ host (include/amt_rccl_collectives.hpp wraps an ncclComm_t),
 *      torch.distributed in the Python mirror (amatsukaze_amd/sharding.py).  Ranks hold contiguous frame ranges in stream
 *      order (rank 0 the first frames).  Both callbacks return 1 on success, 0 on failure. ---- */
typedef struct AmtGpuCollectives {
    int rank, world;
    /* every rank contributes `bytes` bytes; recv receives world*bytes in rank order */
    int (*allgather)(void* user, const void* send, void* recv, int64_t bytes);
    /* in-place sum over all ranks of `count` int64 */
    int (*allreduce_sum_i64)(void* user, int64_t* buf, int64_t count);
    void* user;
} AmtGpuCollectives;

/* LogoFrame::scanFrames sharded (LogoScan.hpp:1577-1584, frames independent): after this rank has scanned its frames
 * [first, first+nlocal) with amtgpu_logoframe_scan_batch, exchange the {corr0,corr1} records so that EVERY rank holds the
 * whole clip's results (8 B per frame per logo) and select_logo / write_result give the single-GPU answer anywhere. */
int  amtgpu_logoframe_allgather_results(AmtGpuLogoFrame* lf, const AmtGpuCollectives* coll, int first, int nlocal);

/* ScanLogo sharded (LogoAnalyzer, LogoScan.hpp:917-1079): dY/dU/dV hold this rank's `nframes_local` frames.  The three
 * globally sequential rounds are kept: round 0 accepts the first numMaxFrames valid frames IN STREAM ORDER (:885; an
 * all-gather of per-rank valid counts gives every rank its share of the quota), each round's exact int64 accumulators are
 * all-reduced, and every rank solves the same regression -> the .lgd is byte-identical to the single-GPU one at any world
 * size.  Rank 0 writes dstpath (other ranks may pass NULL).  A cancel from any rank's callback stops all ranks. */
int  amtgpu_scanlogo_sharded(AmtGpuContext* ctx, const AmtGpuCollectives* coll, const void* dY, const void* dU, const void* dV,
                             int64_t strideY, int64_t strideUV, int pitchY, int pitchUV, int imgw, int imgh,
                             int nframes_local, int serviceid, const char* dstpath, int imgx, int imgy, int w, int h,
                             int thy, int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb);
/* the same for a clip `bits` deep (8..12, the same on every rank), as amtgpu_scanlogo_bits */
int  amtgpu_scanlogo_sharded_bits(AmtGpuContext* ctx, const AmtGpuCollectives* coll, const void* dY, const void* dU, const void* dV,
                                  int64_t strideY, int64_t strideUV, int pitchY, int pitchUV, int imgw, int imgh, int bits,
                                  int nframes_local, int serviceid, const char* dstpath, int imgx, int imgy, int w, int h,
                                  int thy, int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb);

/* The streamed ScanLogo session (amtgpu_scanlogo_stream_create above) frame-sharded: every rank has fed its own contiguous range of
 * the stream into its own session, rank 0 the first frames, each keeping at most numMaxFrames of its own.  An all-gather of the kept counts cuts every rank's store to its share
 * of the first numMaxFrames valid frames of the whole stream, the sums of each round are all-reduced, every rank solves, rank 0
 * writes dstpath (others may pass NULL): the .lgd of one session fed the whole stream.  Failure and cancel on any rank end the call
 * on all, as in amtgpu_scanlogo_sharded. */
int  amtgpu_scanlogo_stream_finish_sharded(AmtGpuScanLogoStream* s, const AmtGpuCollectives* coll, int serviceid, const char* dstpath,
                                           AMTGPU_LOGO_ANALYZE_CB cb);

/* ---- self-specified whole-frame passes (NO in-tree reference arithmetic: SURVEY.md section 0;
 *      "parity unpinned").  Stand in for what chapter_exe (CMAnalyze.hpp:319-337) and KFMDeint's
 *      analysis passes (Misc.cs:1300-1324, FilteredSource.hpp:232-238) compute.  Integer metrics,
 *      specified in DESIGN.md section 6; per frame 8 x uint32/uint64 words, see AMTGPU_FS_*. ---- */
#define AMTGPU_FS_WORDS 8
/* word indices of one frame's record (uint64 each); all sums of absolute sample differences, prev = n-1,
 * vertical metrics over rows 1..H-2, avg(a,c) = (a+c)>>1 */
#define AMTGPU_FS_DIFF_TOP   0   /* sum over even rows |Y_n - Y_prev| */
#define AMTGPU_FS_DIFF_BOT   1   /* sum over odd rows  |Y_n - Y_prev| */
#define AMTGPU_FS_VERT       2   /* sum |Y_n[y-1] - Y_n[y+1]|  (detail inside one field) */
#define AMTGPU_FS_COMB       3   /* sum |Y_n[y] - avg(Y_n[y-1], Y_n[y+1])|  (combing energy of the frame) */
#define AMTGPU_FS_COMB_PREV  4   /* COMB of the weave (even rows of n, odd rows of n-1) */
#define AMTGPU_FS_SUM        5   /* sum of luma */
#define AMTGPU_FS_VERT_PREV  6   /* VERT of that weave */
#define AMTGPU_FS_RESERVED   7
AmtGpuFrameStats* amtgpu_framestats_create(AmtGpuContext* ctx, int width, int height, int bits);
void amtgpu_framestats_destroy(AmtGpuFrameStats* fs);
/* dprevY: Y plane of the frame before the batch (device), or NULL -> frame 0 compares with itself.
 * dout: nframes*AMTGPU_FS_WORDS uint64 (device).  async
 * Frame n lies at dY + n*frame_stride BYTES, its rows `pitch` ELEMENTS apart; dprevY is one frame of the same pitch, anywhere.
 * dY, dprevY, frame_stride and the pitch need to be aligned to the sample size (1 or 2 bytes), nothing more: any pitch >= width,
 * any gap between frames.  Only height * pitch elements of each frame (and of dprevY) are ever read. */
int  amtgpu_framestats_batch(AmtGpuFrameStats* fs, const void* dY, int64_t frame_stride, int pitch,
                             const void* dprevY, int nframes, uint64_t* dout);
/* Frame-sharded runs of the whole-frame passes (fourth row): every rank computes the metrics of its own
 * contiguous frame range [first, first + nlocal) with amtgpu_framestats_batch, passing the frame before its range as dprevY (the
 * one-frame halo: a rank decodes / generates frame first - 1 itself, nothing is exchanged for it; rank 0 passes NULL).  What IS
 * exchanged is the 64-byte record per frame: amtgpu_framestats_allgather takes this rank's records (HOST, nlocal * 8 uint64) and
 * leaves the records of the WHOLE clip (num_frames * 8 uint64, host) in metrics_out on every rank -- ragged shards padded to the
 * largest, ranges checked to tile [0, num_frames) exactly.  The cadence / scene-change decisions (amtgpu_kfm_cadence,
 * amtgpu_cm_scene_changes) then run replicated on every rank from identical input: sequential over the clip, integer only, tiny.
 * A rank-local failure travels as a status word through the exchange; all ranks return 0 together. */
int  amtgpu_framestats_allgather(AmtGpuFrameStats* fs, const AmtGpuCollectives* coll, const uint64_t* local_metrics, int first,
                                 int nlocal, int num_frames, uint64_t* metrics_out);
/* the same for a shard that is resident in HBM as ONE batch: metrics kernel over dY (nlocal frames, dprevY = frame first - 1 or
 * NULL on the rank that holds frame 0), then the exchange.  Synchronises. */
int  amtgpu_framestats_sharded(AmtGpuFrameStats* fs, const AmtGpuCollectives* coll, const void* dY, int64_t frame_stride, int pitch,
                               const void* dprevY, int first, int nlocal, int num_frames, uint64_t* metrics_out);
/* amtgpu_framestats_batch / _sharded on decoder surfaces (AmtGpuSurfaces above: NV12, P010 / P012, planar LSB or MSB).  Only Y, strideY,
 * pitchY, bits and msb_aligned of a descriptor are read: the chroma layout and pointers are ignored.  batch->bits must be the depth the
 * object was created with (8..15: 16-bit surfaces have no metrics).  MSB-aligned containers are read as container >> (16 - bits) inside the
 * kernel, before any arithmetic -- the records are those of the planar LSB clip, whatever sits in the low bits.  prev describes the ONE
 * picture before the batch (its Y plane; same bits, msb_aligned and pitchY as the batch), NULL -> frame 0 compares with itself.
 * nframes == 0 returns 1 and writes nothing; negative nframes returns 0.  async */
int  amtgpu_framestats_surfaces(AmtGpuFrameStats* fs, const AmtGpuSurfaces* batch, const AmtGpuSurfaces* prev, int nframes, uint64_t* dout);
/* amtgpu_framestats_sharded with the shard and the picture before it (a shard that does not start the clip needs prev) as surfaces.
 * Synchronises; a rank-local failure travels through the exchange and all ranks return 0 together. */
int  amtgpu_framestats_sharded_surfaces(AmtGpuFrameStats* fs, const AmtGpuCollectives* coll, const AmtGpuSurfaces* batch,
                                        const AmtGpuSurfaces* prev, int first, int nlocal, int num_frames, uint64_t* metrics_out);
/* host decisions from the metrics of a whole clip (nframes*8 uint64, host): scene-change list in
 * chapter_exe's "SCPos:" sense and per-frame cadence class 0=30i/60p 1=24p(3:2) 2=30p + 3:2 phase.
 * sc_out: up to cap frame numbers, returns count via *nsc.  cadence_out: nframes bytes, phase_out: nframes bytes */
int  amtgpu_cm_scene_changes(const uint64_t* metrics, int nframes, int width, int height, int* sc_out, int cap, int* nsc);
int  amtgpu_kfm_cadence(const uint64_t* metrics, int nframes, int width, int height, uint8_t* cadence_out, uint8_t* phase_out);
/* KFM output-file contract (AMTDecimate, FilteredSource.hpp:645-654): one integer per output frame = how many
 * frames of the 60p clip it spans; sum == 2*nframes.  *nout = output frames written. */
int  amtgpu_kfm_write_durations(const uint8_t* cadence, const uint8_t* phase, int nframes, const char* path, int* nout);
/* KFM timecode contract (readTimecodeFile / readTimecode, FilteredSource.hpp:163-212): "# timecode format v2", one integer
 * start time in ms per output frame, "# total: <seconds>".  fps_num/fps_den = the SOURCE frame rate (30000/1001). */
int  amtgpu_kfm_write_timecode(const uint8_t* cadence, const uint8_t* phase, int nframes, int fps_num, int fps_den, const char* path,
                               int* nout);
/* ---- the pictures of the cadence decisions (self-specified, "parity unpinned": KFMDeint, which renders them in the reference, is not in
 *      the reference tree).  The render plan names, per OUTPUT frame and in the order of the durations file, which
 *      source frames it is made of; amtgpu_kfm_render makes the frames.  The rendered clip is already the decimated one: it needs no
 *      AMTDecimate, its timestamps are amtgpu_kfm_write_timecode's and `ticks` is the durations file.  Top field first. ---- */
typedef struct AmtGpuRenderFrame { int32_t kind, top, bottom, ticks; } AmtGpuRenderFrame;   /* absolute source frame numbers */
#define AMTGPU_RENDER_WEAVE      0   /* even rows from frame `top`, odd rows from frame `bottom` */
#define AMTGPU_RENDER_BOB_TOP    1   /* top == bottom == n: even rows of n kept, odd rows interpolated */
#define AMTGPU_RENDER_BOB_BOTTOM 2   /* top == bottom == n: odd rows of n kept, even rows interpolated */
/* One entry per output frame, walking the clip as amtgpu_kfm_write_durations does (ticks equal its lines entry for entry): a complete
 * 3:2 cycle at n (phases 0..4, all 24p, n + 5 <= nframes) -> WEAVE(n, n) 2, WEAVE(n+1, n+1) 3, WEAVE(top n+3, bottom n+2) 2, WEAVE(n+4, n+4) 3;
 * a 60i frame n -> BOB_TOP(n) 1, BOB_BOTTOM(n) 1; anything else (30p, 24p outside a complete cycle) -> WEAVE(n, n) 2, the frame as it is.
 * *nout = the entries needed; returns 0 when cap is smaller (nothing is written then), 1 otherwise; nframes == 0 returns 1, *nout = 0 */
int  amtgpu_kfm_render_plan(const uint8_t* cadence, const uint8_t* phase, int nframes, AmtGpuRenderFrame* out, int cap, int* nout);
/* ---- source and destination: the one rule of the chain's entry points below -- amtgpu_kfm_render[_deint[_surfaces]], amtgpu_resize_run
 *      [_surfaces], amtgpu_temporal_nr[_surfaces], amtgpu_deband_run[_surfaces], amtgpu_edgelevel -- which all read frames through one AmtGpuSurfaces and write frames
 *      through another.  Each returns 0 with a message on ctx, and launches nothing, unless:
 *   - each descriptor is well formed (not NULL, bits 8..16, MSB-aligned only above 8 bits, reserved 0, no plane NULL but an interleaved
 *     V, strides and plane bases multiples of the container size);
 *   - each is of a layout the call takes: any, or planar LSB-aligned only (interleaved and MSB-aligned descriptors are refused);
 *   - each has the bits the object was created for, where the call has an object (resize, deband);
 *   - no frame stride is negative;
 *   - rows fit their pitch: pitchY >= width, pitchUV >= width / 2 planar and >= width interleaved, where a UV row is `width` containers;
 *   - the two are IN KIND: equal bits, equal interleaved, and an equal shift s = msb_aligned ? 16 - bits : 0.  No call converts layouts;
 *   - a row pitch in bytes fits an int: "pitch above 2 GiB" otherwise, from every one of these calls;
 *   - with more than one destination frame, they do not overlap each other in a plane: each stride is at least (rows - 1) * pitch + row
 *     bytes, luma and chroma;
 *   - no destination plane's byte range (first byte of frame 0 .. last byte of the last frame written) overlaps a source plane's (first
 *     byte of frame 0 .. last byte of the last frame of the batch), over the planes there are: Y and UV when interleaved (V is not
 *     looked at, and may be anything), Y, U and V otherwise.  So no call works in place.
 *      Source and destination may differ in pitch, stride, size (resize) and frame count (render, temporal NR).  The comments below
 *      name only what is particular to each call. ---- */
/* Renders plan[0 .. nout) into dst's frames 0 .. nout - 1.  src holds source frames [src_first, src_first + nsrc) of a clip of clip_frames
 * frames; width x height is the luma size (both even, height >= 4; chroma planes are width / 2 x height / 2); plan is a HOST array.
 * src and dst must be IN KIND: equal bits (8 or 9..16), equal interleaved, and an equal shift s = msb_aligned ? 16 - bits : 0.  Planes in,
 * planes out; NV12 in, NV12 out; P010 / P012 in, the same out; planar MSB in, planar MSB out.  The call converts no layouts (NV12 ->
 * planes, planes -> NV12, MSB -> LSB are refused; amtgpu_weave_fields_batch[_msb] planarises).
 * A missing row y of a BOB entry of frame n, in each plane at its own height:
 *   up = P_n[y-1], dn = P_n[y+1] (a neighbour outside the plane takes the other one's value), spatial = (up + dn + 1) >> 1;
 *   BOB_TOP: a = P_(n-1)[y], b = P_n[y] (n == 0: a = b);  BOB_BOTTOM: a = P_n[y], b = P_(n+1)[y] (n == clip_frames - 1: b = a);
 *   output = thresh >= 0 && |a - b| <= thresh ? (a + b + 1) >> 1 : spatial.
 * thresh is shared by the planes; thresh < 0 is a pure line-average bob that reads no neighbour frame.  No default is recommended: no
 * real footage has been measured.
 * LSB containers (s == 0): up, dn, a, b are the containers as stored, no masking to bits; thresh is in container units.
 * MSB-aligned containers (s > 0): a COPIED row (every row of a WEAVE, the kept rows of a BOB) is the source row's containers as stored,
 * low bits included.  An INTERPOLATED container is computed on samples: up, dn, a, b are container >> s, thresh is in sample units
 * (clamped to (1 << bits) - 1), both means round at the sample's unit, and the stored container is output << s with zero low bits.  So
 * dst >> s is the planar LSB render of src >> s in every container.
 * Interleaved chroma: U is one UV plane of height / 2 rows of `width` containers, pitchUV >= width; V is ignored and may be NULL.  The
 * rule is vertical and temporal only, so each U and each V container meets its own plane's column: the result is the interleave of the
 * planar result.  Y and UV of one allocation (strideY == strideUV == the surface size) is the normal case.
 * Returns 0 with a message on ctx, and launches nothing: what the source and destination rule above refuses (every layout is taken;
 * nsrc source frames, nout destination frames); width or height odd, height < 4; kind outside 0..2; a BOB entry with top != bottom; a
 * frame number outside the batch; thresh >= 0 and a temporal neighbour (n - 1 for BOB_TOP with n >= 1, n + 1 for BOB_BOTTOM with
 * n + 1 < clip_frames) outside the batch.  nout == 0 returns 1.
 * The bytes written depend on the clip and the plan alone: a clip rendered in several calls, each batch with its one-frame halo, gives
 * the bytes of one call.  Reads nothing outside a row's width (width / 2 in planar chroma) containers of a source row, writes nothing
 * outside them in a destination row.  Synchronises: the plan is copied to the device for the one launch and the copy is freed before the
 * call returns */
int  amtgpu_kfm_render(AmtGpuContext* ctx, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height,
                       const AmtGpuRenderFrame* plan, int nout, int thresh, const AmtGpuSurfaces* dst);
/* amtgpu_kfm_render with a choice of the rule that fills a BOB entry's missing rows.  WEAVE entries and the kept rows of a bob are copied
 * exactly as amtgpu_kfm_render copies them under either rule.
 * deint == AMTGPU_DEINT_LINE is amtgpu_kfm_render argument for argument: the same path, the same bytes, surfaces included.
 * deint == AMTGPU_DEINT_ADAPTIVE is an edge-directed, motion-adaptive bob: integer, exact, no threshold.  Each plane
 * by its own width w and height h, containers as stored (no masking to bits), signed integers, >> on non-negative values only.  With
 * C = frame n, P = frame n - 1 (n == 0: C), N = frame n + 1 (n == clip_frames - 1: C), (A, B) = (P, C) for BOB_TOP and (C, N) for
 * BOB_BOTTOM, rows y1m = y-1 >= 0 ? y-1 : y+1, y1p = y+1 < h ? y+1 : y-1, y2m = y-2 >= 0 ? y-2 : y, y2p = y+2 < h ? y+2 : y, columns
 * X(k) = min(max(x + k, 0), w - 1), U = C[y1m], D = C[y1p], a missing row y is per pixel
 *   c = U[x]; e = D[x]; d = (A[y][x] + B[y][x]) >> 1
 *   diff = max(|A[y][x] - B[y][x]| >> 1, (|P[y1m][x] - c| + |P[y1p][x] - e|) >> 1, (|N[y1m][x] - c| + |N[y1p][x] - e|) >> 1)
 *   pred = (c + e) >> 1; score = |U[X(-1)] - D[X(-1)]| + |c - e| + |U[X(1)] - D[X(1)]| - 1
 *   for j = -1, -2 and then for j = +1, +2 (+-2 only where +-1 was taken), against the running score:
 *     s = |U[X(j-1)] - D[X(-j-1)]| + |U[X(j)] - D[X(-j)]| + |U[X(j+1)] - D[X(-j+1)]|;  s < score: score = s, pred = (U[X(j)] + D[X(-j)]) >> 1
 *   b = (A[y2m][x] + B[y2m][x]) >> 1; f = (A[y2p][x] + B[y2p][x]) >> 1
 *   diff = max(diff, min(d - e, d - c, max(b - c, f - e)), -max(d - e, d - c, min(b - c, f - e)))
 *   output = pred clamped into [d - diff, d + diff]   (always inside the container's range: there is no further clamp)
 * Still areas weave (the band closes around the temporal mean d), moving areas interpolate along the edge.  No real footage has been
 * judged: the rule is argued from its construction and a diagonal known answer, not from measured picture quality.
 * ADAPTIVE takes every refusal of amtgpu_kfm_render, and refuses as well: thresh != -1; a deint that is neither constant; a BOB entry
 * whose frame n - 1 (n >= 1) or n + 1 (n + 1 < clip_frames) is outside the batch -- both bobs read both neighbours; and any pair that is
 * not planar and LSB-aligned: this entry point takes planes only under the adaptive rule, and keeps that contract; NV12 / P010 / P012
 * and planar MSB surfaces under the adaptive rule are amtgpu_kfm_render_deint_surfaces below.
 * The bytes depend on the clip and the plan alone: batches with one frame of halo on either side give the bytes of one call.
 * Synchronises, and the plan's device copy lives for the one launch, as amtgpu_kfm_render */
#define AMTGPU_DEINT_LINE     0   /* the rule of amtgpu_kfm_render: line average, temporal mean within thresh */
#define AMTGPU_DEINT_ADAPTIVE 1   /* edge-directed, motion-adaptive; thresh must be -1 */
int  amtgpu_kfm_render_deint(AmtGpuContext* ctx, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height,
                             const AmtGpuRenderFrame* plan, int nout, int deint, int thresh, const AmtGpuSurfaces* dst);
/* amtgpu_kfm_render_deint argument for argument, and the same function behind it, with AMTGPU_DEINT_ADAPTIVE on every pair of surfaces IN
 * KIND (equal bits, interleaved and shift s = msb_aligned ? 16 - bits : 0): NV12, P010 / P012 / P016, interleaved LSB, planar MSB.  A
 * planar LSB pair runs the kernel of amtgpu_kfm_render_deint and gives its bytes; AMTGPU_DEINT_LINE is amtgpu_kfm_render.
 * The result is defined by the planar rule above on samples: de-interleave UV into U and V, each a plane of its own of width / 2 columns
 * with its own column clamp X(k); take samples container >> s; apply the adaptive rule per plane, unchanged (frames n - 1 / n / n + 1,
 * the same row clamps); store an interpolated container as output << s, its low bits zero; re-interleave.  Every COPIED row (all rows of
 * a WEAVE, the kept rows of a BOB) is moved as stored, low bits included, exactly as amtgpu_kfm_render moves it.  An interleaved LSB
 * 16-bit pair and a P016 pair (msb_aligned with bits 16: s = 0) use the containers as stored.  So dst >> s, de-interleaved, is the planar
 * adaptive render of src >> s.  (The rule looks at columns x - 3 .. x + 3, so an interleaved row is NOT walked as one plane of `width`
 * containers as under the line rule: a U container's neighbours are two containers away.)
 * Every refusal of amtgpu_kfm_render_deint is kept, with the same messages, but "planes only": thresh must be -1, a BOB entry needs
 * n - 1 and n + 1 in the batch wherever the clip has them, mixed pairs are refused.  The bytes depend on the clip and the plan alone,
 * with one frame of halo on either side of a batch.  Synchronises */
int  amtgpu_kfm_render_deint_surfaces(AmtGpuContext* ctx, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height,
                                      const AmtGpuRenderFrame* plan, int nout, int deint, int thresh, const AmtGpuSurfaces* dst);
/* ---- temporal noise reduction: TemporalNRFilter (VideoFilter.hpp:27-212), the GUI's EnableTemporalNR, which the server turns into
 *      KTemporalNR(3, 1) (Misc.cs:1425-1428), byte for byte on planar LSB planes.  An addition; the ABI version stays 5. ----
 * src holds frames [src_first, src_first + nsrc) of a clip of clip_frames frames; width x height is the luma size, both even.  Output
 * frames out_first .. out_first + nout - 1 go to dst's frames 0 .. nout - 1.  With d = temporal_distance, N = 2 d + 1,
 * thresh = threshold << (bits - 8), T the container type (uint8_t at bits 8, uint16_t at 9..16; containers as stored, no masking to bits):
 *   the window of output frame t is W_i = frame clamp(t + i - d, 0, clip_frames - 1), i = 0 .. N - 1, a clamped frame counting as often
 *   as it appears; C = W_d = frame t.  Per luma pixel (x, y), cx = x >> 1, cy = interlaced ? (((y >> 1) & ~1) | (y & 1)) : (y >> 1):
 *   diff_i = |C.Y[y][x] - W_i.Y[y][x]| + |C.U[cy][cx] - W_i.U[cy][cx]| + |C.V[cy][cx] - W_i.V[cy][cx]|; W_i passes where diff_i <= thresh;
 *   count = the passing i (the centre always passes); factor = 1.f / (float)count, correctly rounded;
 *   dY = 0.5f, and for i = 0 .. N - 1 in order, where W_i passes, dY += factor * (float)W_i.Y[y][x] -- the product rounded to float, then
 *   the sum, no fused operation; dU, dV likewise from the pixel's chroma samples;  dst.Y[y][x] = (T)dY by truncation;
 *   where x is even and ((interlaced ? y >> 1 : y) & 1) == 0 also dst.U[cy][cx] = (T)dU and dst.V[cy][cx] = (T)dV: a chroma sample is
 *   filtered with the pass mask of ONE luma pixel, (2 cx, 2 cy) progressive and (2 cx, 2 (cy & ~1) + (cy & 1)) interlaced.
 * Every container of the nout output frames is written; none is copied from the source.  The reference's onFrame / finish stream gives
 * exactly these windows for clip_frames >= 2 d (and clip_frames == 1 with d == 0); for shorter clips it drops frames, which this call
 * does not mirror: the clamp rule holds for every length.
 * The bytes depend on the clip and the parameters alone: a clip filtered in batches, each with d frames of halo wherever the clip has
 * them, gives the bytes of one call.
 * Returns 0 with a message on ctx, and launches nothing: temporal_distance outside 0..63; threshold outside 0..32767; bits outside 8..16;
 * what the source and destination rule above refuses (planar LSB only; nsrc source frames, nout destination frames); width or height
 * odd; interlaced with height % 4 != 0 (the reference reads chroma row height / 2 there); a window frame outside the batch; an output
 * frame outside the clip.  nout == 0 returns 1.
 * Reads nothing outside a row's width (width / 2 in chroma) containers of a source row, writes nothing outside them in a destination row.
 * Synchronises, as amtgpu_kfm_render does: dst is complete when the call returns */
int  amtgpu_temporal_nr(AmtGpuContext* ctx, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height,
                        int out_first, int nout, int temporal_distance, int threshold, int interlaced, const AmtGpuSurfaces* dst);
/* The same filter on decoder surfaces where they lie, source and destination IN KIND -- equal bits, equal interleaved, equal MSB shift:
 * NV12 (8 bits, interleaved), P010 / P012 / P016 (interleaved, MSB-aligned), interleaved LSB at 9..16 bits, planar MSB at 9..16 bits;
 * a planar LSB pair runs amtgpu_temporal_nr's kernel unchanged.  An addition; the ABI version stays 5.  The parameters are
 * amtgpu_temporal_nr's.  The rule is the one above, stated on samples: sample = container >> s, s = msb_aligned ? 16 - bits : 0;
 * thresh = threshold << (bits - 8) counts samples; U is the even and V the odd container of an interleaved UV row (pitchUV >= width).
 * Every container of the nout output frames is written as result << s, its low bits zero; nothing is copied from the source, so the
 * source's low bits never survive.  So dst >> s, de-interleaved, equals amtgpu_temporal_nr of src >> s, de-interleaved, byte for byte,
 * whatever sits in the source's low bits and however the clip is cut into batches with temporal_distance frames of halo.
 * Every refusal of amtgpu_temporal_nr is kept, with its wording, but "planar LSB only": a mixed pair is refused instead ("not in kind
 * ... converts no layouts"), as the source and destination rule has it for every layout.  Synchronises */
int  amtgpu_temporal_nr_surfaces(AmtGpuContext* ctx, const AmtGpuSurfaces* src, int src_first, int nsrc, int clip_frames, int width, int height,
                                 int out_first, int nout, int temporal_distance, int threshold, int interlaced, const AmtGpuSurfaces* dst);

/* ---- resize: the BlackmanResize(w, h) in front of KTemporalNR in the server's chain (Misc.cs:1423; the GUI's "resize" checkbox), on
 *      planar LSB planes in HBM.  Self-specified, "parity unpinned" (BlackmanResize is a built-in of the AviSynth host; its arithmetic
 *      is not in the reference tree): integer and exact, so the bytes are those of the rule below wherever it
 *      runs.  An addition; the ABI version stays 5. ----
 * One axis, S source samples to D destination samples, kernel k with `taps`, everything in double on the host:
 *   scale = D / S, fstep = min(scale, 1), support = taps / fstep, K0 = ceil(2 * support), K = min(K0, S);
 *   k(x) = 0 for |x| >= taps, 1 at 0, else with px = pi |x|:  blackman (default taps 4) sin(px)/px * (0.42 + 0.5 cos(px/taps) + 0.08 cos(2 px/taps));
 *   lanczos (default taps 3) sin(px)/px * sin(px/taps)/(px/taps);  bilinear max(0, 1 - |x|), taps 1.
 *   Output sample i: c = (i + 0.5) / scale - 0.5, lo = floor(c - support) + 1; for p = lo .. lo + K0 - 1 the weight k((p - c) * fstep) is
 *   added to position clamp(p, 0, S - 1) (the edge sample replicated, folded on the host); the weights are divided by their sum; each
 *   becomes C = floor(w * 16384 + 0.5); the residual 16384 - sum(C) is added to the largest C, the lowest position among equals;
 *   start = clamp(lo, 0, S - K).  The axis' program is start[D] and C[D][K], C[i][j] belonging to source position start[i] + j.
 * Sample rule: out = clamp((sum_j C[i][j] * s[start[i] + j] + 8192) >> 14, 0, maxv), int32 accumulator, arithmetic shift,
 *   maxv = (1 << bits) - 1.
 * Frame rule: the horizontal stage runs on every source row into an intermediate of dst_w x src_h samples, rounded and clamped as above,
 *   at the clip's depth; the vertical stage runs on the intermediate.  Every plane on its own: chroma is S/2 -> D/2 with the same kernel,
 *   chroma siting is ignored.  Frames are independent: the bytes do not depend on how a clip is cut into calls.  Equal sizes copy.
 * amtgpu_resize_create: all four sizes even and positive, bits 8..16, kernel one of AMTGPU_RESIZE_*; taps <= 0 takes the kernel's default
 *   (at most 64).  max_scratch_bytes bounds the intermediate the object owns, whatever the clip's length: a call works through its
 *   frames in rounds of as many frames as fit it, at least one; <= 0 takes AMTGPU_RESIZE_DEFAULT_SCRATCH_BYTES.  Returns NULL with a
 *   message on ctx: a figure below one frame's intermediate (rows of dst_w samples rounded up to 16 bytes, src_h of them, plus the two
 *   chroma planes'); a program whose largest sum of positive coefficients times maxv plus 8192, or likewise of negative ones, leaves
 *   int32; a horizontal window (K samples) that does not fit the kernel's staging region (2000 bytes).
 * amtgpu_resize_run: frames 0 .. nframes - 1 of src (src_w x src_h) into frames 0 .. nframes - 1 of dst (dst_w x dst_h), planar LSB planes
 *   of the resizer's bits.  Returns 0 with a message on ctx, and launches nothing: what the source and destination rule above refuses
 *   (planar LSB only; the resizer's bits, so unequal bits too; each side by its own size; nframes frames on either side).
 *   nframes == 0 returns 1.  Reads nothing outside a row's width of a source row, writes nothing outside it in a destination
 *   row; the source is never written.  All rounds run in the context's stream.  Synchronises, as amtgpu_temporal_nr does.
 * amtgpu_resize_run_surfaces: the same object, rounds, scratch bound and checks on decoder surfaces where they lie, source and
 *   destination IN KIND: equal bits (the resizer's), interleaved and msb_aligned -- NV12, interleaved LSB, P010 / P012 / P016, planar MSB.
 *   With s = msb_aligned ? 16 - bits : 0, U the even and V the odd container of a UV row: a sample is container >> s (the source's low
 *   bits are dropped on the way in); the rule above runs on the samples, every plane on its own, chroma per component with the chroma
 *   programs; every destination container is result << s.  The resize copies no row, so no low bit survives, at equal sizes either (the
 *   program is then a single 16384).  Hence dst >> s, de-interleaved, is amtgpu_resize_run of src >> s, de-interleaved, byte for byte,
 *   whatever the low bits hold and however the call is cut into rounds.  A planar LSB pair runs amtgpu_resize_run's kernels and gives
 *   its bytes.  An interleaved UV row is `width` containers, and pitchUV at least that.  Returns 0 with a message on ctx, and launches
 *   nothing: what amtgpu_resize_run refuses, the layout apart; a pair that is not in kind (no layout is converted); on interleaved
 *   surfaces, a chroma window whose K pairs of 2 containers do not fit the staging region (2000 bytes: half the samples a planar chroma
 *   row may take -- such an object still runs planar surfaces).  An addition; the ABI version stays 5.
 * amtgpu_resize_get_program: K, start[D] and coeff[D * K] of plane 0 (luma) / 1 (chroma), axis 0 (horizontal) / 1 (vertical); start and
 *   coeff may be NULL, so that a caller can ask for K first (D is the destination size of that plane and axis) */
typedef struct AmtGpuResize AmtGpuResize;
#define AMTGPU_RESIZE_BLACKMAN 0
#define AMTGPU_RESIZE_LANCZOS  1
#define AMTGPU_RESIZE_BILINEAR 2
#define AMTGPU_RESIZE_DEFAULT_SCRATCH_BYTES (64ll << 20)     /* 64 MiB: a quarter of the 256 MiB last-level cache of an MI355X */
AmtGpuResize* amtgpu_resize_create(AmtGpuContext* ctx, int src_w, int src_h, int dst_w, int dst_h, int bits, int kernel, int taps,
                                   int64_t max_scratch_bytes);
void amtgpu_resize_destroy(AmtGpuResize* r);
int  amtgpu_resize_run(AmtGpuResize* r, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes);
int  amtgpu_resize_run_surfaces(AmtGpuResize* r, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes);
int  amtgpu_resize_get_program(AmtGpuResize* r, int plane, int axis, int* K, int* start, int* coeff);

/* ---- deband: the KDeband(25, 1, 2, true) behind KTemporalNR in the server's chain (Misc.cs:1431; the GUI's "banding reduction"
 *      checkbox, which the reference's README pairs with the temporal NR), on planar LSB planes (amtgpu_deband_run) or decoder surfaces
 *      in kind (amtgpu_deband_run_surfaces) in HBM.  Self-specified, "parity
 *      unpinned" (KDeband belongs to AviSynthCUDAFilters; its source is not in the reference tree): integer and
 *      exact, so the bytes are those of the rule below wherever it runs and depend on the clip and the parameters alone.  The argument
 *      order (range, threshold, sample, blur_first) and the defaults 25, 1, 2, true are the server's call.  An addition; the ABI
 *      version stays 5. ----
 * Planes of 8..16 bits, 4:2:0, width and height even.  Every plane is filtered on its own and every frame on its own; there is no halo
 * in time, so a clip cut into calls gives the bytes of one call.  For plane p (0 Y, 1 U, 2 V) of Wp x Hp containers, radius the caller's
 * figure (KDeband's range, 1..31), Rp = radius for luma and radius >> 1 for chroma:
 *   lim(x, y) = min(Rp, x, Wp - 1 - x, y, Hp - 1 - y): no reference sample ever lies outside the plane.
 *   The offset table is static over frames and built on the host, once per object, everything uint32 with wrap-around:
 *     mix(v): v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b; v ^= v >> 16;
 *     key_p = mix(seed + 0x9e3779b9 * (p + 1));  h = mix(key_p ^ (y << 16 | x));  a = h & 255, b = (h >> 8) & 255;
 *     dx = ((a * (2 lim + 1)) >> 8) - lim,  dy = ((b * (2 lim + 1)) >> 8) - lim: both int8 in [-lim, lim].
 *   The references of a pixel: p0 = s[y + dy][x + dx], p1 = s[y - dy][x - dx], p2 = s[y + dx][x - dy], p3 = s[y - dx][x + dy] -- p2, p3
 *     are the pair p0, p1 turned by 90 degrees; |dx|, |dy| <= lim keeps all four inside the plane.
 *   With c = s[y][x] and thresh = threshold << (bits - 8) (the temporal NR's scaling; threshold 0..32767):
 *     sample 0: out = p0 if |p0 - c| <= thresh, else c;
 *     sample 1: avg = (p0 + p1 + 1) >> 1;  sample 2: avg = (p0 + p1 + p2 + p3 + 2) >> 2;
 *     blur_first non-zero: out = avg if |avg - c| <= thresh, else c;  zero: out = avg if every |p_i - c| <= thresh, else c.
 *   Containers are taken as stored (no masking to bits), as in the temporal NR.  There is no grain and no dither.
 * amtgpu_deband_create: the object owns the three planes' offset tables on the device.  Returns NULL with a message on ctx: an odd or
 *   non-positive size, or one above 65534 (the hash key packs y << 16 | x); bits outside 8..16; radius outside 1..31; threshold outside
 *   0..32767; sample outside 0..2.
 * amtgpu_deband_run: frames 0 .. nframes - 1 of src into frames 0 .. nframes - 1 of dst, planar LSB planes of the object's size and
 *   bits, in one launch.  Returns 0 with a message on ctx, and launches nothing: what the source and destination rule above refuses
 *   (planar LSB only; the object's bits; nframes frames on either side) -- in-place is impossible here, the filter reads neighbours.
 *   nframes == 0 returns 1.  Reads nothing outside the first Wp
 *   containers of a source row and writes nothing outside them in a destination row; every container of the output frames is written;
 *   the source is never written.  Synchronises, as amtgpu_resize_run does.
 * amtgpu_deband_run_surfaces: the same call on decoder surfaces IN KIND -- NV12, interleaved 16-bit LSB, P010 / P012 / P016, planar
 *   16-bit MSB -- where they lie; a P010 chain needs no planar copy in front of the deband and none behind it.  The rule is the rule
 *   above, on samples.  With s = 16 - bits where the pair is MSB-aligned, else 0: a sample is container >> s, whatever the low bits
 *   hold; thresh = threshold << (bits - 8) counts samples; in an interleaved UV row U is the even container and V the odd one, and the
 *   two stay as independent as planes: U is filtered with plane 1's table and V with plane 2's, each with radius >> 1 and lim(x, y) of
 *   the W/2 x H/2 component plane, and a reference of a U container is a U container.  Every container of every row is written and no
 *   row is copied, so every destination container is result << s, its low bits zero, as in the resize.  The contract: dst >> s,
 *   de-interleaved, is byte for byte what amtgpu_deband_run gives for src >> s, de-interleaved, for the same object.  The checks are
 *   amtgpu_deband_run's with every layout taken, and the pair must be in kind ("the filter converts no layouts").  A planar LSB pair
 *   launches amtgpu_deband_run's kernel and gives its bytes.  The object keeps, besides the three tables, U's and V's interleaved (U's
 *   entry at 2x, V's at 2x + 1); amtgpu_deband_set_offsets on plane 1 or 2 rebuilds it.  An addition; the ABI version stays 5.
 * amtgpu_deband_get_offsets: plane p's table, Wp * Hp int8 each, row-major (either pointer may be NULL).
 * amtgpu_deband_set_offsets: replaces one plane's table with the caller's -- a pattern of the caller's own, or a test's planted one.
 *   Refused, the table staying as it was, if any |dx| or |dy| exceeds lim(x, y).  Synchronises */
typedef struct AmtGpuDeband AmtGpuDeband;
AmtGpuDeband* amtgpu_deband_create(AmtGpuContext* ctx, int width, int height, int bits, int radius, int threshold, int sample, int blur_first,
                                   uint32_t seed);
void amtgpu_deband_destroy(AmtGpuDeband* d);
int  amtgpu_deband_run(AmtGpuDeband* d, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes);
int  amtgpu_deband_run_surfaces(AmtGpuDeband* d, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int nframes);
int  amtgpu_deband_get_offsets(AmtGpuDeband* d, int plane, int8_t* dx, int8_t* dy);          /* Wp * Hp each, row-major */
int  amtgpu_deband_set_offsets(AmtGpuDeband* d, int plane, const int8_t* dx, const int8_t* dy);

/* ---- edge level: the KEdgeLevel(16, 10, 2) behind KDeband in the server's chain (Misc.cs:1435; the GUI's "edge enhancement (for
 *      anime)" checkbox), on planar LSB planes in HBM.  Self-specified, "parity unpinned" (KEdgeLevel belongs to AviSynthCUDAFilters; its
 *      source is not in the reference tree; the reference's README describes it as a port of AviUtl's edge-level filter that leaves out
 *      edges that are already sharp and areas that are too blurred and applies its result through a step like RgTools' Repair; DESIGN.md
 *      section 6g): integer and exact, so the bytes are those of the rule below wherever it runs and depend on the clip and the
 *      parameters alone.  The rule is this project's; its constants are the specification's own, and no real footage has been judged.
 *      The argument order (str, thrs, repair) and the defaults 16, 10, 2 are the server's call.  An addition; the ABI version stays 5. ----
 * - Input is planar LSB planes of 8..16 bits, 4:2:0, `width` and `height` even and positive.
 * - Frames are independent: there is no halo in time, and a clip cut into calls gives the bytes of one call.
 * - Chroma is copied.  Every container of U and V goes to the destination as stored.  AviUtl's filter is luma only, and KEdgeLevel's
 *   call passes no chroma argument.
 * - Containers are taken as stored, with no masking to `bits`, as in the temporal NR and the deband.
 * Parameters, in the server's order (str, thrs, repair): strength 0..255; threshold 0..32767, with T = threshold << (bits - 8);
 * repair 0..4.  For the luma sample c = s[y][x]:
 * 1. Border.  Where x < 2, x >= W - 2, y < 2 or y >= H - 2: out = c.  No reference ever lies outside the plane, so there is no edge
 *    rule.  A plane narrower or lower than 5 is copied.
 * 2. Direction.  H5 = s[y][x-2 .. x+2], V5 = s[y-2 .. y+2][x].  rh = max(H5) - min(H5), rv = max(V5) - min(V5).  The line L is V5
 *    where rh < rv, else H5.  A tie takes the horizontal line.  mx = max(L), mn = min(L), rng = mx - mn.
 * 3. Flat.  rng <= T: out = c.
 * 4. Step.  step = max |L[i+1] - L[i]|, i = 0..3.  Sharp already: 4 * step >= 3 * rng: out = c.  Too blurred: 8 * step <= 3 * rng:
 *    out = c.  A linear ramp has 4 * step = rng.
 * 5. Level.  avg = (mx + mn) >> 1.  e = c + (((c - avg) * strength) >> 4), the shift arithmetic (floor).  e is clamped into [mn, mx].
 *    |c - avg| <= 32768 and strength <= 255, so the product is below 2^23 in magnitude: a signed 24-bit multiply holds it.
 * 6. Repair.  With repair = r > 0: sort the nine source samples s[y-1..y+1][x-1..x+1] ascending as n[0..8].
 *    out = min(max(e, n[r - 1]), n[9 - r]).  These are RgTools' Repair modes 1..4, the source as its own reference.  With r = 0:
 *    out = e.  Repair is applied only where step 5 was reached.  It can move a pixel that step 5 left at c.
 * amtgpu_edgelevel: frames 0 .. nframes - 1 of src into frames 0 .. nframes - 1 of dst, in one launch for all three planes.  Stateless,
 *   like amtgpu_temporal_nr: there is no table, so no object.  Returns 0 with a message on ctx, and launches nothing: strength,
 *   threshold or repair out of range; a negative frame count; an odd or non-positive size; what the source and destination rule above
 *   refuses (planar LSB only: decoder surfaces in kind are not built; bits that differ between the sides; nframes frames on either
 *   side) -- in-place is impossible here, the filter reads neighbours.  nframes == 0 returns 1.  Reads nothing outside the first
 *   `width` (`width / 2`) containers of a source row and writes nothing outside them in a destination row; every container of the
 *   output frames is written; the source is never written.  Synchronises: dst is complete when the call returns */
int  amtgpu_edgelevel(AmtGpuContext* ctx, const AmtGpuSurfaces* src, const AmtGpuSurfaces* dst, int width, int height, int nframes, int strength,
                      int threshold, int repair);

/* chapter_exe output contract (CMAnalyze::readSceneChanges, CMAnalyze.hpp:411-439): header, a "----" line, "SCPos: <frame>"
 * lines.  This call writes no "mute" lines: amtgpu_cm_write_chapter_exe_mute below writes the file with them */
int  amtgpu_cm_write_chapter_exe(const int* scene_changes, int nsc, int nframes, const char* path);

/* ---- per-video-frame audio levels, mute sections and chapter_exe's "mute" lines (self-specified, "parity unpinned": chapter_exe's
 *      source is not in the reference tree).  PCM is interleaved little-endian int16, `channels` (1..8) elements
 *      per sample-frame.  Video frame n owns sample-frames [b(n), b(n + 1)), b(n) = floor(n * sample_rate * fps_den / fps_num) in int64
 *      (the VideoInfo::AudioSamplesFromFrames contract); positions >= num_samples do not exist: they add nothing and are not counted.
 *      Per frame 4 x uint64, exact integers, independent of how the stream is cut into calls. ---- */
typedef struct AmtGpuAudioLevels AmtGpuAudioLevels;
#define AMTGPU_AL_WORDS  4      /* uint64 each */
#define AMTGPU_AL_PEAK   0      /* max |s| over the span; |-32768| = 32768 */
#define AMTGPU_AL_SUMABS 1      /* sum |s| */
#define AMTGPU_AL_SUMSQ  2      /* sum s*s */
#define AMTGPU_AL_COUNT  3      /* int16 elements of the span that lie inside the timeline */
/* NULL with a message on ctx: sample_rate, fps_num or fps_den not positive, channels outside 1..8, negative num_samples */
AmtGpuAudioLevels* amtgpu_audiolevels_create(AmtGpuContext* ctx, int sample_rate, int channels, int fps_num, int fps_den, int64_t num_samples);
void    amtgpu_audiolevels_destroy(AmtGpuAudioLevels* al);
/* b(frame); -1 for a negative frame or a position beyond 63 bits */
int64_t amtgpu_audiolevels_frame_start(const AmtGpuAudioLevels* al, int64_t frame);
/* Records of video frames [first_frame, first_frame + nframes) into d_out (device, nframes * AMTGPU_AL_WORDS uint64).  d_pcm (device)
 * holds sample-frames [pcm_first, pcm_first + pcm_count) of the timeline and must cover
 * [b(first_frame), min(b(first_frame + nframes), num_samples)), else the call is refused; nothing outside that part of d_pcm is read.
 * d_pcm needs 2-byte alignment and nothing more.  nframes == 0 returns 1 and writes nothing.  async */
int     amtgpu_audiolevels_batch(AmtGpuAudioLevels* al, const int16_t* d_pcm, int64_t pcm_first, int64_t pcm_count,
                                 int first_frame, int nframes, uint64_t* d_out);
/* The same records for the audio of an amts file into h_out (HOST): the wave file is read through amtgpu_amts_read_audio in chunks of a
 * few thousand video frames, uploaded through the pinned staging ring and reduced chunk by chunk.  The object must have been created
 * with channels == 2 (the reference's assembly is 16-bit stereo).  Synchronises */
int     amtgpu_audiolevels_amts(AmtGpuAudioLevels* al, const AmtGpuAmtsFile* a, const char* wavepath,
                                int first_frame, int nframes, uint64_t* h_out);
/* Mute sections from the records of a whole clip (host): a frame is silent iff PEAK <= mute_level or COUNT == 0; a section is a maximal
 * run of at least min_frames (>= 1) silent frames, reported as inclusive [start_out[i], end_out[i]].  *nmute = the total; returns 1 iff
 * the total is at most cap (the first cap sections are written either way), as amtgpu_cm_scene_changes does */
int amtgpu_cm_mute_sections(const uint64_t* levels, int nframes, int mute_level, int min_frames,
                            int* start_out, int* end_out, int cap, int* nmute);
/* amtgpu_cm_write_chapter_exe's file with the format's other half: after the header and the "----" line, in ascending frame order, one
 * "mute%2d: %d - %d" line per section (numbered from 1) in front of every scene change >= its start, and the "\tSCPos: %d %d" lines.  A
 * scene change belongs to a section when start <= sc <= end + 1 (a cut on the first sounding frame is the section's).  only_muted == 0:
 * every scene change is written -- CMAnalyze::readSceneChanges builds the list it builds from amtgpu_cm_write_chapter_exe's file;
 * only_muted != 0: scene changes that belong to no section are dropped.  0: scene changes not ascending, sections not ascending,
 * overlapping, with start > end or reaching outside [0, nframes), or a file that cannot be written */
int amtgpu_cm_write_chapter_exe_mute(const int* scene_changes, int nsc, const int* mute_start, const int* mute_end, int nmute,
                                     int nframes, int only_muted, const char* path);

/* ---- automatic logo detection (self-specified, "parity unpinned": no reference arithmetic).  The reference
 *      needs a rectangle drawn by hand before ScanLogo (LogoScan.hpp:1083-1098); these entry points find it from the clip.
 *      Over the Y planes of all frames offered, per pixel: S1 = sum Y, SM = sum (|Y[x+1]-Y[x-1]| + |Y[y+1]-Y[y-1]|) (0 on the outer
 *      ring), N = frames.  The summed gradient (from S1) against SM gives a coherence in [0, 1] -- static edges such as a logo's add
 *      up, moving content does not; coherent strong edges are joined into ranked candidate rectangles.  All sums are int64 and
 *      exact: independent of frame order, batch split and GPU count. ---- */
typedef struct AmtGpuLogoFind AmtGpuLogoFind;
typedef struct AmtGpuLogoFindParams {
    float min_coherence;    /* edge pixel: coherence m / SM at least this (default 0.6) */
    float min_edge;         /* ... and persistent edge strength m / N at least this, in 8-bit LSB units (default 3) */
    int   join;             /* dilation radius (pixels, square) that merges the strokes of one logo (default 4) */
    int   margin;           /* the rectangle is the edge pixels' bounding box grown by this on each side (default 4) */
    int   min_w, min_h;     /* smallest bounding box kept (default 16 x 16) */
    float max_w_frac, max_h_frac;   /* largest bounding box kept, as a fraction of the frame (default 0.5 x 0.5) */
} AmtGpuLogoFindParams;
/* one candidate: imgx, imgy even, w, h even, inside the frame (the reference's LogoHeader keeps all four even, LogoScan.hpp:69).
 * score = sum of m / N over its edge pixels (input sample units); coherence = sum m / sum SM over them; ranked by score, descending,
 * ties by (imgy, imgx) */
typedef struct AmtGpuLogoRect {
    int   imgx, imgy, w, h;
    float score, coherence;
    int   edge_pixels, reserved;
} AmtGpuLogoRect;
/* width, height >= 3, bits 8..16.  NULL on failure (message on the context) */
AmtGpuLogoFind* amtgpu_logofind_create(AmtGpuContext* ctx, int width, int height, int bits);
void amtgpu_logofind_destroy(AmtGpuLogoFind* lf);
/* adds the Y planes of nframes frames (device; frame n at dY + n*frame_stride bytes, pitch in ELEMENTS as everywhere in this header,
 * uint8 for 8 bits, uint16 containers above) to the sums.  Batches of any length: the driver splits them into launches whose 32-bit
 * partials cannot overflow.  dY, frame_stride and the pitch need to be aligned to the sample size, nothing more (any pitch >= width,
 * any gap between frames); only height * pitch elements of each frame are ever read.  async */
int  amtgpu_logofind_add_batch(AmtGpuLogoFind* lf, const void* dY, int64_t frame_stride, int pitch, int nframes);
/* the same from decoder surfaces (AmtGpuSurfaces: only Y, strideY, pitchY, bits and msb_aligned are read; bits must be the finder's).  The
 * sums of MSB-aligned input are those of the shifted samples container >> (16 - bits), exact as ever.  async */
int  amtgpu_logofind_add_surfaces(AmtGpuLogoFind* lf, const AmtGpuSurfaces* batch, int nframes);
int64_t amtgpu_logofind_nframes(const AmtGpuLogoFind* lf);
/* sums: 2*W*H int64 (host), S1 then SM, row-major.  get synchronises; set replaces the sums and the frame count (nframes >= 0) */
int  amtgpu_logofind_get_sums(AmtGpuLogoFind* lf, int64_t* sums);
int  amtgpu_logofind_set_sums(AmtGpuLogoFind* lf, const int64_t* sums, int64_t nframes);
void amtgpu_logofind_default_params(AmtGpuLogoFindParams* params);
/* ranked candidates from the current sums: the best min(cap, total) go to out, *ncand = total.  params NULL = defaults */
int  amtgpu_logofind_candidates(AmtGpuLogoFind* lf, const AmtGpuLogoFindParams* params, AmtGpuLogoRect* out, int cap, int* ncand);
/* the same from sums in host memory, no device: sums = 2*W*H int64 as above.  Refuses NULL sums / ncand (out may be NULL only when
 * cap == 0), W or H below 3, bits outside 8..16, nframes < 0, cap < 0 and parameters out of range.  Returns 0 without a message
 * (there is no context). */
int  amtgpu_logofind_candidates_host(const int64_t* sums, int width, int height, int bits, int64_t nframes, const AmtGpuLogoFindParams* params,
                                     AmtGpuLogoRect* out, int cap, int* ncand);
/* frame-sharded detection: every rank has added its own frames; one allreduce_sum_i64 over the 2*W*H + 1 values (the frame count rides
 * along) leaves identical sums on every rank.  Synchronises. */
int  amtgpu_logofind_allreduce(AmtGpuLogoFind* lf, const AmtGpuCollectives* coll);
/* ScanLogo without a rectangle: detection over all nframes frames (8-bit; _auto_bits below for 9..12), then amtgpu_scanlogo with the best
 * candidate, which *found receives (may be NULL).  No candidate: returns 0 with "no logo found", *found zeroed, no file written. */
int  amtgpu_scanlogo_auto(AmtGpuContext* ctx, const void* dY, const void* dU, const void* dV, int64_t strideY, int64_t strideUV,
                          int pitchY, int pitchUV, int imgw, int imgh, int nframes, int serviceid, const char* dstpath, int thy,
                          int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb, const AmtGpuLogoFindParams* params, AmtGpuLogoRect* found);
/* the same for a clip `bits` deep (8..12): the detection runs at that depth, then amtgpu_scanlogo_bits */
int  amtgpu_scanlogo_auto_bits(AmtGpuContext* ctx, const void* dY, const void* dU, const void* dV, int64_t strideY, int64_t strideUV,
                               int pitchY, int pitchUV, int imgw, int imgh, int bits, int nframes, int serviceid, const char* dstpath, int thy,
                               int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb, const AmtGpuLogoFindParams* params, AmtGpuLogoRect* found);
/* the same over frame-sharded ranks: each adds its own frames, the sums are all-reduced (every rank finds the same rectangle), then
 * amtgpu_scanlogo_sharded.  Rank 0 writes dstpath. */
int  amtgpu_scanlogo_auto_sharded(AmtGpuContext* ctx, const AmtGpuCollectives* coll, const void* dY, const void* dU, const void* dV,
                                  int64_t strideY, int64_t strideUV, int pitchY, int pitchUV, int imgw, int imgh, int nframes_local,
                                  int serviceid, const char* dstpath, int thy, int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb,
                                  const AmtGpuLogoFindParams* params, AmtGpuLogoRect* found);
int  amtgpu_scanlogo_auto_sharded_bits(AmtGpuContext* ctx, const AmtGpuCollectives* coll, const void* dY, const void* dU, const void* dV,
                                       int64_t strideY, int64_t strideUV, int pitchY, int pitchUV, int imgw, int imgh, int bits,
                                       int nframes_local, int serviceid, const char* dstpath, int thy, int numMaxFrames,
                                       AMTGPU_LOGO_ANALYZE_CB cb, const AmtGpuLogoFindParams* params, AmtGpuLogoRect* found);
/* amtgpu_scanlogo_file without a rectangle: the raw clip ('AMTR', or 'AMTH' for 9..12 bits) is read twice -- detection over the Y planes of every frame (through
 * the pinned upload path), then amtgpu_scanlogo_file with the best candidate */
int  amtgpu_scanlogo_file_auto(AmtGpuContext* ctx, const char* srcpath, int serviceid, const char* workfile, const char* dstpath, int thy,
                               int numMaxFrames, AMTGPU_LOGO_ANALYZE_CB cb, const AmtGpuLogoFindParams* params, AmtGpuLogoRect* found);

#ifdef __cplusplus
}
#endif
#endif /* AMT_GPU_H */
