// eval_pair_body.h -- the body of the scan's two-fade evaluation kernels, shared by its two forms: eval_pair_kernels.hip (two staging
// units per lane over the tile's whole box, a second staging pass for tiles of more than 64 units) and eval_pair1_kernels.hip (one
// listed unit per lane on the single-pass plans of eval_tiles.hpp).  What the kernels compute and why they are shaped this way:
// eval_pair_kernels.hip.
#pragma once
#include "build_knobs.h"
#include <hip/hip_runtime.h>
#include <cstdint>
#include <algorithm>
#include <type_traits>

#include "engine.hpp"
#include "eval_tiles.hpp"
#include "exact_math.h"
#include "eval_tile_stage.h"
#include "eval_ordered_sum.h"

namespace amt {

using namespace lin;
using namespace tile;

constexpr int pair_threads(int nw) { return (nw + 1) * 64; }                          // the evaluation waves + the summing wave
constexpr int pair_row_pitch(int nw) { return nw * kTileLanes + kEvalScorePad; }      // floats; the sum reads ahead of the row's end
constexpr int kPairThreads = pair_threads(kTileWaves);

// {corr(k, s), corr(k, bg)} around the window means M = window_means(W) in the reference's order (exact_math.h corr5x5_strided),
// both halves at once
__device__ __forceinline__ f2 window_corr_exact(const f2 (&Kp)[13], const f2 (&W)[25], f2 M)
{
    f2 p[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        f2 t[5];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const int e = r * 5 + i;
            const f2 kk = (e & 1) ? bc_hi(Kp[e >> 1]) : bc_lo(Kp[e >> 1]);
            t[r] = kk * (W[e] - M);
        }
        p[i] = ((t[0] + t[1]) + (t[2] + t[3])) + t[4];
    }
    return ((p[0] + p[4]) + p[2]) + (p[1] + p[3]);
}

// bin of CorrelationScore (LogoScan.hpp:304), (int)clamp(mean, 0, 255) >> 3; the clamp in front of the conversion bounds what is
// converted (pair_eligible keeps |bg| below 2^30 so that it is finite at all).  STAGE4: `mean` is four times the window mean
// (eval_tile_stage.h Quad) -- floor(4 m) >> 5 == floor(m) >> 3 for m in [0, 255] (both are floor(m / 8)), and anything above
// clamps to bin 31 either way (1020 >> 5 == 255 >> 3 == 31)
template <bool STAGE4> __device__ __forceinline__ unsigned score_bin_bounded(float mean)
{
    return STAGE4 ? (unsigned)((int)__builtin_amdgcn_fmed3f(mean, 0.0f, 1020.0f) >> 5) : (unsigned)((int)__builtin_amdgcn_fmed3f(mean, 0.0f, 255.0f) >> 3);
}

struct PairLaunch {
    const EvalLogoDev* logos;
    const TileLogoDev* tls;
    const void* Y;
    const int* frame_map;
    long long frame_stride;      // elements
    int pitch;                   // elements
    float maxv;
    int nframes, G, ngroups, nlogos;
    float* out;
    int out_frame_stride, take_abs;
};

#ifdef AMT_PAIR_OCC
#define AMT_PAIR_OCC_ATTR __attribute__((amdgpu_waves_per_eu(AMT_PAIR_OCC, AMT_PAIR_OCC)))
#else
#define AMT_PAIR_OCC_ATTR
#endif
// STAGE4: the logos' tables carry the 0.25 of DeintY (taps scaled on the host: EvalEngine::ensure_tiles) and the tile planes hold
// {4 s, 4 bg} -- no v_ldexp_f32 per staged sample; records are the same bits (eval_tile_stage.h Quad).  An engine with a logo whose
// tables cannot be scaled runs the other instance (logo_eval_pair_ldexp_kernel) on unscaled tables.
//
// ONE_UNIT: the engine's plans are single-pass ones (eval_tiles.hpp kTileCutUnits).  A lane stages ONE unit, the one the plan lists for
// it (TileLogoDev::units, a word per slot): three raw loads per request instead of six, no second staging pass, and the unit's row
// and column come out of the word instead of the u / ncol4 arithmetic.  The word is a vector load that all of a tile's addresses
// depend on, so it is fetched a band ahead, at a band's end where the next band's pixel and taps are requested, and made a plain
// value there (the terms' flush has just waited for everything older, the word is the first load behind it): the loop carries a
// register, no load crosses the back edge, and no wait stands between the next tile's coefficient loads and its raw request.
//
// NW: the evaluation waves of the instance = the tiles per band of the plans it walks (TilePlan::waves; the shapes: eval_tiles.hpp
// tile_pair_shape)
template <typename pix_t, bool STAGE4, bool ONE_UNIT = false, int NW = kTileWaves>
__device__ __forceinline__ void logo_eval_pair_body(const PairLaunch& A)
{
    constexpr int kPairRowPitch = pair_row_pitch(NW);
    extern __shared__ float lds[];
    f2* const planes = reinterpret_cast<f2*>(lds);                       // [NW][kTileCap] {s, bg}: a wave's own tile
    float* const rows = lds + NW * kTileCap * 2;                         // [2][2 G][kPairRowPitch] per-pixel terms of a band

    const int G = A.G;
    const WgMap wm = wg_map_shared_rows((int)blockIdx.x, A.nlogos, A.ngroups);
    if (wm.grp >= A.ngroups) return;                               // (the grid is whole blocks of eight groups; a whole workgroup leaves: no barrier is missed)
    const int logo = wm.logo, grp = wm.grp;
    const int F0 = grp * G;
    const int gcount = min(G, A.nframes - F0);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const EvalLogoDev* const Lp = A.logos + logo;
    const TileLogoDev* const Xp = A.tls + logo;
    const int nbands = Xp->nbands;

    if (wave == NW) {
        // ---------------- the summing wave: after the barrier that ends band b it adds band b's rows ----------------
        // Its chain of dependent adds is short on instructions but long on latency: with the issue priority raised it gets its
        // slot as soon as an add's operand is ready instead of queueing behind the SIMD's evaluation waves for every element
        // (measured: 18.7 -> 10 cycles per element), and the band's rows are free again long before the next barrier.
        __builtin_amdgcn_s_setprio(3);
        float acc = 0.0f;
        typedef const __attribute__((address_space(4))) TileBandDesc* const_band_ptr;
        const const_band_ptr bd = (const_band_ptr)Xp->bands;
        for (int b = 0; b < nbands; ++b) {
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            const int npix = bd[b].npix;
            if (lane < 2 * gcount) acc = ordered_row_sum(rows + ((b & 1) * 2 * G + lane) * kPairRowPitch, npix, acc);
        }
        if (lane < 2 * gcount) {
            float r = acc / Lp->blackScore;
            if (A.take_abs) r = fabsf(r);
            A.out[(long long)(F0 + (lane >> 1)) * A.out_frame_stride + Lp->out_off + (lane & 1)] = r;
        }
        return;
    }

    // ---------------- evaluation waves ----------------
    typedef const __attribute__((address_space(4))) TileLogoDev* tlogo_ptr;          // (wave-uniform table bases: scalar loads, once)
    const gptr_t gSc = (gptr_t)Xp->sc, gK = (gptr_t)((tlogo_ptr)Xp)->kp, gInfo = (gptr_t)((tlogo_ptr)Xp)->sinfo;
    const unsigned nslots8 = (unsigned)Xp->nslots * 8u;
    const const_tile_ptr tiles = (const_tile_ptr)(Xp->tiles + wave);
    f2* const myplane = planes + wave * kTileCap;
    const unsigned plane_base = lds_address(myplane);
    typename std::conditional<ONE_UNIT, TileStager1<pix_t, STAGE4>, TileStager<pix_t, STAGE4>>::type st;
    st.init(Lp, A.pitch, A.maxv, myplane);
    TilePixel px;

    TileDesc T;
    fetch_tile(T, tiles);
    // (ONE_UNIT) the unit word of this lane in the NEXT tile of the wave; past the last band the last band's again, which nobody uses
    gptr_t gUnits = nullptr;
    unsigned unext = 0;
    if constexpr (ONE_UNIT) {
        gUnits = (gptr_t)((tlogo_ptr)Xp)->units;
        st.setup_units(T, gld<unsigned>(gUnits, ((unsigned)wave * 64u + (unsigned)lane) * 4u));
    } else {
        st.setup_units(T, lane);
    }
    st.request(frame_rsrc<pix_t>(A.Y, A.frame_map, A.frame_stride, F0));
    // (the first raw samples must not be the LAST loads issued before the loop: vector-memory loads return in order, and the wait the
    //  compiler places at the loop head for them is the merge of this path and the back edge -- with the raw loads sunk below the 14
    //  pixel / tap loads it became vmcnt(0) in every iteration, which also waits for the scale gathers issued just before)
    asm volatile("" ::: "memory");
    if constexpr (ONE_UNIT) unext = gld<unsigned>(gUnits, ((unsigned)((nbands > 1 ? NW : 0) + wave) * 64u + (unsigned)lane) * 4u);
    px.load(gK, gInfo, nslots8, (unsigned)wave * 64u + (unsigned)lane, T, plane_base);
    if constexpr (ONE_UNIT) asm volatile("" : "+v"(unext));
    st.coefs_landed();

    // the terms of an evaluation are formed one iteration later, when its two scale gathers have long arrived
    f2 pR = {0.0f, 0.0f}, psc0 = pR, psc1 = pR;
    int prow = 0;                    // (scalar) the pending terms' first row: 2 * frame in the band's set of rows
    bool pact = false;
    auto flush_terms = [&]() {
        if (pact) {
            float* const pdst = rows + prow * kPairRowPitch + px.ridx;
            pdst[0] = score_term(pR.x, psc0.x, psc0.y);               // LogoScan.hpp:305-308
            pdst[kPairRowPitch] = score_term(pR.y, psc1.x, psc1.y);
        }
    };

    int b = 0, g = 0;
    const int niter = nbands * gcount;
    for (int it = 0; it < niter; ++it) {
        const bool band_end = g + 1 == gcount;
        // ---- 1. the iteration's tile: raw -> {s, bg} pairs in this wave's plane ----
        st.convert();
        // ---- 2. the next iteration's raw samples travel during the evaluation (past the last iteration: a repeat nobody reads) ----
        if (band_end && b + 1 < nbands) {
            fetch_tile(T, tiles + (b + 1) * NW);
            if constexpr (ONE_UNIT) st.setup_units(T, unext);
            else st.setup_units(T, lane);
        }
        st.request(frame_rsrc<pix_t>(A.Y, A.frame_map, A.frame_stride, F0 + (band_end ? 0 : g + 1)));
        // ---- 3. both fades of the frame: one packed window evaluation ----
        // (the taps are loop-invariant: LICM would hoist their {k,k} broadcasts and keep 50 registers of copies; the empty asm
        //  makes them opaque per iteration and the broadcast folds into the multiply's op_sel)
#pragma unroll
        for (int j = 0; j < 13; ++j) asm volatile("" : "+v"(px.Kp[j]));
        f2 W[25];
        unsigned wrow[5];
        px.rows(wrow);
        const f2 M = window_load_means(wrow, W);      // (issuing the reads before the next requests instead: 2.630 ms either way, round 5)
        const f2 R = window_corr_exact(px.Kp, W, M);
        // ---- 4. the previous iteration's terms -> the band's score rows, at the pixel's raster position; then this iteration's two
        //      scale gathers go straight into the registers the terms were read from (a copy would wait for them here) ----
        flush_terms();
        psc0 = gld<f2>(gSc, __umul24(score_bin_bounded<STAGE4>(M.x), nslots8) + px.slot8);
        psc1 = gld<f2>(gSc, __umul24(score_bin_bounded<STAGE4>(M.y), nslots8) + px.slot8);
        pR = R; pact = px.act;
        prow = (b & 1) * 2 * G + g * 2;
        if (band_end) {
            flush_terms();                                           // the band's rows are complete before the waves meet
            pact = false;
            // the band's last evaluation is done.  Its terms have just waited for their scale gathers and, as vector-memory loads return in
            // order, for the next tile's logo coefficients (requested in step 2, a whole evaluation ago): b * maxv is formed here
            // without a wait of its own.  Then the next band's pixel and taps travel across the barrier
            ++b; g = 0;
            if (b < nbands) {
                st.coefs_landed();
                if constexpr (ONE_UNIT) unext = gld<unsigned>(gUnits, ((unsigned)((b + 1 < nbands ? b + 1 : b) * NW + wave) * 64u + (unsigned)lane) * 4u);
                px.load(gK, gInfo, nslots8, (unsigned)(b * NW + wave) * 64u + (unsigned)lane, T, plane_base);
                if constexpr (ONE_UNIT) asm volatile("" : "+v"(unext));
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        } else {
            ++g;
        }
    }
}

// the launch arguments both forms share; hipSuccess with *grid == 0: nothing to launch
inline hipError_t pair_launch_args(PairLaunch& A, size_t* lds, unsigned* grid, int bits, const EvalLogoDev* dlogos, const TileLogoDev* dtls, int nlogos,
                                   const FrameBatch& luma, const int* dframe_map, int nframes, int G, float* dout, int out_frame_stride, int take_abs,
                                   int nw = kTileWaves)
{
    *grid = 0; *lds = 0;
    if (nframes <= 0 || nlogos <= 0) return hipSuccess;
    if (luma.shift || luma.es != (bits <= 8 ? 1 : 2)) return hipErrorInvalidValue;
    A.logos = dlogos; A.tls = dtls; A.Y = luma.Y; A.frame_map = dframe_map; A.frame_stride = luma.strideY / luma.es; A.pitch = luma.pitchY;
    A.maxv = (float)((1 << bits) - 1);
    A.nframes = nframes; A.G = G; A.ngroups = (nframes + G - 1) / G; A.nlogos = nlogos;
    A.out = dout; A.out_frame_stride = out_frame_stride; A.take_abs = take_abs;
    *lds = tile_pair_lds_bytes(nw, G, kEvalScorePad);
    if (G < 1 || 2 * G > 64 || *lds > 160 * 1024) return hipErrorInvalidValue;
    *grid = (unsigned)wg_grid_shared_rows(A.ngroups, nlogos);
    return hipSuccess;
}

} // namespace amt
