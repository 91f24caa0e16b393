"""Writes tests/golden/temporal_nr_v1.npz: inputs and outputs of the reference's own TemporalNRFilter (Amatsukaze/VideoFilter.hpp).

The class is compiled where it lies, with g++ -O2 -ffp-contract=off, against two stand-in headers (Transcode.hpp, CudaFilter.h: an
av::Frame over a plain AVFrame, the pixel-format descriptor, THROW, inline cudaTNR* stubs) and a small driver that pushes a clip through
onFrame / finish and writes down what comes out.  The stand-ins and the driver are this file's own text; nothing of the reference is
copied.  Everything is built in a temporary directory outside the tree (VideoFilter.hpp is reached through a symbolic link there, so
that its quoted includes find the stand-ins first).

Run by hand where the reference tree is at hand; nothing in build(), the tests, smoke() or bench.py calls it:
    python tools/make_temporal_nr_golden.py --reference /path/to/reference [--out tests/golden/temporal_nr_v1.npz]

The golden holds, per case cK: cK_params = (bits, temporal_distance, threshold, interlaced), the clip cK_Y / _U / _V, the emitted frames
cK_oY / _oU / _oV and their frame numbers cK_idx -- and short5_idx / short3_idx, the frame numbers the reference emits for a clip of 5
and of 3 frames at temporal_distance 3 (it drops frames of clips shorter than 2 * temporal_distance)."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

TRANSCODE_HPP = r"""
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

struct NonCopyable {
    NonCopyable() {}
    NonCopyable(const NonCopyable&) = delete;
    NonCopyable& operator=(const NonCopyable&) = delete;
};

enum AVPixelFormat { AV_PIX_FMT_NONE = -1, AV_PIX_FMT_YUV420P, AV_PIX_FMT_YUV420P10LE, AV_PIX_FMT_YUV420P12LE, AV_PIX_FMT_YUV420P14LE, AV_PIX_FMT_YUV420P16LE };
struct AVFrame {
    uint8_t* data[4];
    int linesize[4];
    int format, width, height;
    std::vector<uint8_t> store;
};
struct AVComponentDescriptor { int depth; };
struct AVPixFmtDescriptor { AVComponentDescriptor comp[4]; };
inline const AVPixFmtDescriptor* av_pix_fmt_desc_get(AVPixelFormat f)
{
    static const AVPixFmtDescriptor d[5] = {{{{8}, {8}, {8}, {0}}}, {{{10}, {10}, {10}, {0}}}, {{{12}, {12}, {12}, {0}}}, {{{14}, {14}, {14}, {0}}}, {{{16}, {16}, {16}, {0}}}};
    return &d[(int)f];
}
inline int av_frame_copy_props(AVFrame*, const AVFrame*) { return 0; }
inline int av_frame_get_buffer(AVFrame* f, int align)
{
    const int es = f->format == AV_PIX_FMT_YUV420P ? 1 : 2;
    size_t total = 0, at[3];
    for (int p = 0; p < 3; ++p) {
        const int w = p ? f->width / 2 : f->width, h = p ? f->height / 2 : f->height;
        f->linesize[p] = (w * es + align - 1) / align * align;
        at[p] = total;
        total += (size_t)f->linesize[p] * h;
    }
    f->store.assign(total, 0xCD);
    for (int p = 0; p < 3; ++p) f->data[p] = f->store.data() + at[p];
    return 0;
}

namespace av {
class Frame {
public:
    explicit Frame(int index) : frameIndex_(index), frame_() {}
    Frame(const Frame& o) : frameIndex_(o.frameIndex_), frame_(o.frame_)
    {
        for (int p = 0; p < 3; ++p) frame_.data[p] = frame_.store.data() + (o.frame_.data[p] - o.frame_.store.data());
    }
    AVFrame* operator()() { return &frame_; }
    int frameIndex_;
private:
    AVFrame frame_;
};
}

#define THROW(type, message) throw std::runtime_error(#type)
"""

CUDAFILTER_H = r"""
#pragma once
typedef void* CudaTNRFilter;
inline CudaTNRFilter cudaTNRCreate(int, int, int, int) { return nullptr; }
inline int cudaTNRSendFrame(CudaTNRFilter, AVFrame*) { return -1; }
inline int cudaTNRRecvFrame(CudaTNRFilter, AVFrame*) { return -1; }
inline int cudaTNRFinish(CudaTNRFilter) { return -1; }
"""

DRIVER_CPP = r"""
// usage: driver in out bits distance threshold interlaced frames width height
// in: tight Y, U, V planes per frame; out: int32 count, then per emitted frame int32 frameIndex and tight Y, U, V planes
#include <cstdio>
#include "VideoFilter.hpp"

struct Collect : VideoFilter {
    std::vector<std::unique_ptr<av::Frame>> got;
    void start() {}
    void onFrame(std::unique_ptr<av::Frame>&& f) { got.emplace_back(std::move(f)); }
    void finish() {}
};

int main(int argc, char** argv)
{
    if (argc != 10) return 2;
    const int bits = atoi(argv[3]), d = atoi(argv[4]), thr = atoi(argv[5]), il = atoi(argv[6]), n = atoi(argv[7]), w = atoi(argv[8]), h = atoi(argv[9]);
    const int es = bits <= 8 ? 1 : 2;
    const AVPixelFormat fmt = bits == 8 ? AV_PIX_FMT_YUV420P : bits == 10 ? AV_PIX_FMT_YUV420P10LE : bits == 12 ? AV_PIX_FMT_YUV420P12LE
                            : bits == 14 ? AV_PIX_FMT_YUV420P14LE : AV_PIX_FMT_YUV420P16LE;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    TemporalNRFilter filter;
    Collect sink;
    filter.init(d, thr, il != 0);
    filter.nextFilter = &sink;
    filter.start();
    for (int i = 0; i < n; ++i) {
        std::unique_ptr<av::Frame> f(new av::Frame(i));
        AVFrame* a = (*f)();
        a->format = fmt; a->width = w; a->height = h;
        av_frame_get_buffer(a, 64);
        for (int p = 0; p < 3; ++p)
            for (int y = 0; y < (p ? h / 2 : h); ++y)
                if (fread(a->data[p] + (size_t)a->linesize[p] * y, es, p ? w / 2 : w, in) != (size_t)(p ? w / 2 : w)) return 4;
        filter.onFrame(std::move(f));
    }
    filter.finish();
    const int32_t count = (int32_t)sink.got.size();
    fwrite(&count, 4, 1, out);
    for (auto& f : sink.got) {
        const int32_t idx = f->frameIndex_;
        fwrite(&idx, 4, 1, out);
        AVFrame* a = (*f)();
        for (int p = 0; p < 3; ++p)
            for (int y = 0; y < (p ? h / 2 : h); ++y) fwrite(a->data[p] + (size_t)a->linesize[p] * y, es, p ? w / 2 : w, out);
    }
    fclose(out);
    return 0;
}
"""

# (bits, temporal_distance, threshold, interlaced, frames, width, height)
CASES = [
    (8, 3, 1, 0, 12, 34, 8),
    (10, 1, 1, 1, 6, 18, 8),
    (14, 3, 1, 1, 6, 10, 8),           # exactly 2 d frames
    (16, 0, 2, 0, 3, 6, 4),
    (16, 3, 2, 0, 10, 18, 4),
    (8, 1, 3, 1, 5, 34, 8),
]
SHORT = {"short5_idx": 5, "short3_idx": 3}      # frames of the two short clips at temporal_distance 3


def build_driver(reference, tmp):
    for name, text in (("Transcode.hpp", TRANSCODE_HPP), ("CudaFilter.h", CUDAFILTER_H), ("driver.cpp", DRIVER_CPP)):
        with open(os.path.join(tmp, name), "w") as f:
            f.write(text)
    os.symlink(os.path.join(os.path.abspath(reference), "Amatsukaze", "VideoFilter.hpp"), os.path.join(tmp, "VideoFilter.hpp"))
    exe = os.path.join(tmp, "driver")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++14", "-w", "-I", tmp, os.path.join(tmp, "driver.cpp"), "-o", exe])
    return exe


def run_reference(exe, tmp, planes, bits, d, threshold, interlaced):
    """(frame numbers, Y, U, V) of what the reference emits for the clip"""
    Y, U, V = planes
    n, h, w = Y.shape
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        for i in range(n):
            for p in (Y, U, V):
                f.write(np.ascontiguousarray(p[i]).tobytes())
    subprocess.check_call([exe, src, dst] + [str(v) for v in (bits, d, threshold, interlaced, n, w, h)])
    raw = open(dst, "rb").read()
    count = int(np.frombuffer(raw, np.int32, 1)[0])
    dt, es = Y.dtype, Y.dtype.itemsize
    fb = (w * h + 2 * (w // 2) * (h // 2)) * es
    assert len(raw) == 4 + count * (4 + fb), (len(raw), count)
    idx, out = [], ([], [], [])
    for k in range(count):
        at = 4 + k * (4 + fb)
        idx.append(int(np.frombuffer(raw, np.int32, 1, at)[0]))
        at += 4
        for p, (hh, ww) in enumerate(((h, w), (h // 2, w // 2), (h // 2, w // 2))):
            out[p].append(np.frombuffer(raw, dt, hh * ww, at).reshape(hh, ww))
            at += hh * ww * es
    stack = lambda a, hh, ww: np.stack(a) if a else np.zeros((0, hh, ww), dt)
    return np.array(idx, np.int32), stack(out[0], h, w), stack(out[1], h // 2, w // 2), stack(out[2], h // 2, w // 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds Amatsukaze/VideoFilter.hpp)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "temporal_nr_v1.npz"))
    args = ap.parse_args()
    import temporal_nr_ref as R
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(args.reference, tmp)
        for k, (bits, d, thr, il, n, w, h) in enumerate(CASES):
            planes = R.make_clip(n, w, h, bits, thr, np.random.default_rng(1000 + k))
            if bits == 10:
                planes[0][1, 2, 3] = 0xFC00                  # containers above maxv are taken as stored
                planes[1][2, 1, 1] = 0x0FFF
            idx, oY, oU, oV = run_reference(exe, tmp, planes, bits, d, thr, il)
            res.update({f"c{k}_params": np.array([bits, d, thr, il], np.int32), f"c{k}_Y": planes[0], f"c{k}_U": planes[1], f"c{k}_V": planes[2],
                        f"c{k}_idx": idx, f"c{k}_oY": oY, f"c{k}_oU": oU, f"c{k}_oV": oV})
            print(f"case {k}: bits {bits} d {d} threshold {thr} interlaced {il}, {n} frames of {w}x{h}: emitted {idx.tolist()}", file=sys.stderr)
        for name, n in SHORT.items():
            planes = R.make_clip(n, 6, 4, 8, 1, np.random.default_rng(7))
            res[name] = run_reference(exe, tmp, planes, 8, 3, 1, 0)[0]
            print(f"{name}: {res[name].tolist()}", file=sys.stderr)
    np.savez_compressed(args.out, **res)
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
