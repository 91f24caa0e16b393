// frame_batch.h -- FrameBatch, the one description of a batch of frames that every launcher takes (kernels.hpp), on its own and without
// HIP: host code that only checks a batch (plane_pair.hpp) includes this file and is compiled and tested with plain g++.
#pragma once

#include <cstdint>

namespace amt {

// A batch of 4:2:0 frames in HBM, the one description every launcher takes.  Strides (between frames) are in BYTES, as the ABI counts them;
// pitches (between rows) in containers of es bytes.  interleaved: U is the U0 V0 U1 V1 ... plane and V unused; sample = container >> shift.
// Planar LSB planes are interleaved = 0, shift = 0.  A kernel whose argument list counts strides in samples gets stride / es on the line
// that forms that argument, and nowhere else.  Built by plane_batch / surface_batch (api_common.hpp), which refuse what es does not divide.
// A luma batch (frame metrics, logo finder, evaluation kernels) has U = V = nullptr, strideUV = pitchUV = 0; its launchers read Y, strideY,
// pitchY, es and shift alone (an NV12 surface's Y plane is a Y plane), and an es that is not their `bits`' container size is hipErrorInvalidValue.
struct FrameBatch { const void *Y, *U, *V; long long strideY, strideUV; int pitchY, pitchUV; int es, interleaved, shift; };
// the same batch from frame `frames` on
inline FrameBatch plane_batch_from(FrameBatch b, long long frames)
{
    auto at = [&](const void* p, long long stride) { return (const void*)((const uint8_t*)p + frames * stride); };
    b.Y = at(b.Y, b.strideY); b.U = at(b.U, b.strideUV); b.V = at(b.V, b.strideUV);
    return b;
}

} // namespace amt
