// cs_gray4.h -- the gray depth of a [N,H,W,C] float32 frame as the depth pre-passes read it (cs_temporal.hip, cs_depthrange.hip;
// cs_guideddepth.hip takes the choice of the access path).  The passes run in a chain and must agree bit for bit on this map, so it
// is defined here and nowhere else.
//
// The contract.  A lane owns the four consecutive pixels i .. i + 3 of a frame of hw pixels, i a multiple of 4:
//   C == 3 (CM 3)      gray_of(r, g, b) of the pixel's three channels (cs_common.h: the warp's own gray expression)
//   C == 1 (CM 1)      the value itself
//   any other C (CM 0) channel 0 of the pixel's c channels
//   a pixel at or behind hw reads as 0 and is never written
//   VEC true   16-byte accesses.  The caller guarantees hw % 4 == 0 (so i + 3 < hw wherever i < hw) and the frame's first element on
//              the 16-byte grid (vec4_path below); CM 0 has no such form, its channel 0 is strided.
//   VEC false  the same four pixels through guarded 4-byte accesses: the same values on either path.
#pragma once
#include <initializer_list>

#include "cs_common.h"

namespace cs {

struct Px4 { float v[4]; };

template <int CM, bool VEC>
__device__ __forceinline__ Px4 load_gray4(const float* frame, size_t i, size_t hw, int c) {
    Px4 g;
    if (VEC && CM == 1) {
        const float4 a = *reinterpret_cast<const float4*>(frame + i);
        g.v[0] = a.x; g.v[1] = a.y; g.v[2] = a.z; g.v[3] = a.w;
    } else if (VEC && CM == 3) {
        const float4* q = reinterpret_cast<const float4*>(frame + 3 * i);
        const float4 a = q[0], b = q[1], cc = q[2];
        g.v[0] = gray_of(a.x, a.y, a.z); g.v[1] = gray_of(a.w, b.x, b.y);
        g.v[2] = gray_of(b.z, b.w, cc.x); g.v[3] = gray_of(cc.y, cc.z, cc.w);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const size_t p = i + k;
            float x = 0.0f;
            if (p < hw) {
                if (CM == 1) x = frame[p];
                else if (CM == 3) x = gray_of(frame[3 * p], frame[3 * p + 1], frame[3 * p + 2]);
                else x = frame[p * (size_t)c];
            }
            g.v[k] = x;
        }
    }
    return g;
}

// the four pixels of a one-channel frame, written as load_gray4<1, VEC> reads them
template <bool VEC>
__device__ __forceinline__ void store4(float* frame, size_t i, size_t hw, const Px4& g) {
    if (VEC) {
        *reinterpret_cast<float4*>(frame + i) = make_float4(g.v[0], g.v[1], g.v[2], g.v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (i + k < hw) frame[i + k] = g.v[k];
    }
}

// ---- host: the choice of the path -----------------------------------------------------------------------------------------------
inline bool on16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The 16-byte path: `px` -- the pixels between two starts of a lane's groups of four: a frame's h * w, or a row's w for a pass that
// works row by row -- is a multiple of 4, and every listed buffer starts on the 16-byte grid.
inline bool vec4_path(size_t px, std::initializer_list<const void*> bufs) {
    bool vec = (px & 3) == 0;
    for (const void* p : bufs) vec = vec && on16(p);
    return vec;
}

}  // namespace cs
