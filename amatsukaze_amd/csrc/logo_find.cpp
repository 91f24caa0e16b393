// logo_find.cpp -- automatic logo detection, host half: from the edge-persistence sums (logofind_kernels.hip) to ranked candidate
// rectangles.  Self-specified, no reference arithmetic.  No device.
#include "build_knobs.h"
#include "../../include/amt_gpu.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

bool params_ok(const AmtGpuLogoFindParams& p)
{
    return p.min_coherence >= 0.f && p.min_coherence <= 1.f && p.min_edge >= 0.f && p.join >= 0 && p.join <= 64 && p.margin >= 0 &&
           p.min_w >= 1 && p.min_h >= 1 && p.max_w_frac > 0.f && p.max_w_frac <= 1.f && p.max_h_frac > 0.f && p.max_h_frac <= 1.f;
}

// square dilation of radius r, separable: a running count over each row, then over each column
std::vector<uint8_t> dilate(const std::vector<uint8_t>& m, int W, int H, int r)
{
    if (r == 0) return m;
    std::vector<uint8_t> t((size_t)W * H, 0), o((size_t)W * H, 0);
    for (int y = 0; y < H; ++y) {
        const uint8_t* s = &m[(size_t)y * W];
        int cnt = 0;
        for (int x = 0; x < std::min(W, r); ++x) cnt += s[x];
        for (int x = 0; x < W; ++x) {
            if (x + r < W) cnt += s[x + r];
            if (x - r - 1 >= 0) cnt -= s[x - r - 1];
            t[(size_t)y * W + x] = cnt > 0;
        }
    }
    for (int x = 0; x < W; ++x) {
        int cnt = 0;
        for (int y = 0; y < std::min(H, r); ++y) cnt += t[(size_t)y * W + x];
        for (int y = 0; y < H; ++y) {
            if (y + r < H) cnt += t[(size_t)(y + r) * W + x];
            if (y - r - 1 >= 0) cnt -= t[(size_t)(y - r - 1) * W + x];
            o[(size_t)y * W + x] = cnt > 0;
        }
    }
    return o;
}

} // namespace

extern "C" {

void amtgpu_logofind_default_params(AmtGpuLogoFindParams* p)
{
    if (!p) return;
    p->min_coherence = 0.6f;
    p->min_edge = 3.0f;
    p->join = 4;
    p->margin = 4;
    p->min_w = 16;
    p->min_h = 16;
    p->max_w_frac = 0.5f;
    p->max_h_frac = 0.5f;
}

int amtgpu_logofind_candidates_host(const int64_t* sums, int W, int H, int bits, int64_t nframes, const AmtGpuLogoFindParams* params,
                                    AmtGpuLogoRect* out, int cap, int* ncand)
{
    try {
        AmtGpuLogoFindParams P;
        amtgpu_logofind_default_params(&P);
        if (params) P = *params;
        if (!sums || !ncand || (cap > 0 && !out) || W < 3 || H < 3 || bits < 8 || bits > 16 || nframes < 0 || cap < 0 || !params_ok(P))
            return 0;
        *ncand = 0;
        if (nframes == 0) return 1;
        const int64_t* S1 = sums;
        const int64_t* SM = sums + (size_t)W * H;
        const double invN = 1.0 / (double)nframes, to8 = 255.0 / (double)((1 << bits) - 1);
        // 1. edge pixels: coherent (m / SM) and persistent (m / N) summed gradient, interior only
        std::vector<uint8_t> edge((size_t)W * H, 0);
        std::vector<double> mag((size_t)W * H, 0.0);
        for (int y = 1; y < H - 1; ++y)
            for (int x = 1; x < W - 1; ++x) {
                const size_t i = (size_t)y * W + x;
                if (SM[i] <= 0) continue;
                const double gx = (double)(S1[i + 1] - S1[i - 1]), gy = (double)(S1[i + W] - S1[i - W]);
                const double m = std::sqrt(gx * gx + gy * gy);
                if (m >= (double)P.min_coherence * (double)SM[i] && m * invN * to8 >= (double)P.min_edge) {
                    edge[i] = 1;
                    mag[i] = m;
                }
            }
        // 2-3. joined strokes -> 8-connected components of the dilated mask
        const std::vector<uint8_t> joined = dilate(edge, W, H, P.join);
        std::vector<int> label((size_t)W * H, -1);
        std::vector<int> stack;
        struct Comp { int x0, y0, x1, y1, n; double m, sm; };
        std::vector<Comp> comps;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t i0 = (size_t)y * W + x;
                if (!joined[i0] || label[i0] >= 0) continue;
                const int id = (int)comps.size();
                Comp c{W, H, -1, -1, 0, 0.0, 0.0};
                label[i0] = id;
                stack.assign(1, (int)i0);
                while (!stack.empty()) {
                    const int i = stack.back();
                    stack.pop_back();
                    const int px = i % W, py = i / W;
                    if (edge[i]) {         // 4-5. the box, count and score of the ORIGINAL edge pixels
                        c.x0 = std::min(c.x0, px); c.x1 = std::max(c.x1, px);
                        c.y0 = std::min(c.y0, py); c.y1 = std::max(c.y1, py);
                        ++c.n;
                        c.m += mag[i];
                        c.sm += (double)SM[i];
                    }
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) {
                            const int qx = px + dx, qy = py + dy;
                            if (qx < 0 || qy < 0 || qx >= W || qy >= H) continue;
                            const size_t q = (size_t)qy * W + qx;
                            if (joined[q] && label[q] < 0) { label[q] = id; stack.push_back((int)q); }
                        }
                }
                comps.push_back(c);
            }
        // 4, 6. size limits on the edge box; the rectangle = box + margin, corners even, clipped to the frame
        std::vector<AmtGpuLogoRect> cand;
        for (const Comp& c : comps) {
            if (c.n == 0) continue;
            const int bw = c.x1 - c.x0 + 1, bh = c.y1 - c.y0 + 1;
            if (bw < P.min_w || bh < P.min_h || bw > (double)P.max_w_frac * W || bh > (double)P.max_h_frac * H) continue;
            const int x0 = std::max(0, c.x0 - P.margin) & ~1, y0 = std::max(0, c.y0 - P.margin) & ~1;
            const int x1 = std::min(W, c.x1 + 1 + P.margin), y1 = std::min(H, c.y1 + 1 + P.margin);
            int w = (x1 - x0 + 1) & ~1, h = (y1 - y0 + 1) & ~1;
            if (x0 + w > W) w -= 2;          // an odd frame width cuts the rounded-up rectangle: the last whole pair
            if (y0 + h > H) h -= 2;
            if (w <= 0 || h <= 0) continue;
            AmtGpuLogoRect r;
            r.imgx = x0; r.imgy = y0; r.w = w; r.h = h;
            r.score = (float)(c.m * invN);
            r.coherence = c.sm > 0 ? (float)(c.m / c.sm) : 0.f;
            r.edge_pixels = c.n;
            r.reserved = 0;
            cand.push_back(r);
        }
        // 7. by score, descending; ties by (imgy, imgx)
        std::sort(cand.begin(), cand.end(), [](const AmtGpuLogoRect& a, const AmtGpuLogoRect& b) {
            if (a.score != b.score) return a.score > b.score;
            if (a.imgy != b.imgy) return a.imgy < b.imgy;
            if (a.imgx != b.imgx) return a.imgx < b.imgx;
            if (a.w != b.w) return a.w < b.w;
            return a.h < b.h;
        });
        *ncand = (int)cand.size();
        for (int i = 0; i < (int)cand.size() && i < cap; ++i) out[i] = cand[i];
        return 1;
    } catch (...) {
        return 0;
    }
}

} // extern "C"
