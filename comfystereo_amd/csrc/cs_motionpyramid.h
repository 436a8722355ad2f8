// cs_motionpyramid.h -- what the host and the device share of the coarse-to-fine motion search (cs_motionpyramid.hip, cs_abi.hip):
// the planes' geometry, the packed key of the refinement's order, the range of search_range and the workspace's blocks.  Plain C++
// but for the __host__ __device__ marks, so a stand-alone host program can check it (tests/test_motion_pyramid_surface.py).
#pragma once
#include "cs_motiondepth.h"

namespace cs {

enum {
    MP_LEVELS = 3,           // planes 0 (the luma), 1 and 2
    MP_MIN_R = 4,            // search_range: a multiple of MP_STEP_R from MP_MIN_R to MP_MAX_R; the coarse range is R / 4 <= 30 <= MD_MAX_S
    MP_MAX_R = 120,
    MP_STEP_R = 4,
    MP_WAVES = MD_THREADS / 64,   // blocks a workgroup of the refinement serves, a wave each
    MP_PARENTS = 5,          // the parent and its up, down, left and right neighbours
    MP_WINDOWS = MP_PARENTS + 1,  // their 18 x 18 reference windows and the one of (0, 0)
    MP_CANDS = 9 * MP_PARENTS + 1,   // 46: 2 v + (ex, ey) per parent, then (0, 0)
    MP_WIN_ROWS = MD_BLOCK + 2,   // 18
    MP_WIN_DW = 6,           // 18 columns and up to 3 of alignment: 21 bytes, and the read ahead of the fifth dword stays inside 24
    MP_WIN_PITCH = 7,        // dwords per staged row: odd, so the 16 rows a candidate's lanes read lie on 16 banks
    MP_BIAS = 128,
};

// The order (cost, |dx| + |dy|, |dy|, dy, dx) as one integer: cost << 31 | (|dx| + |dy|) << 23 | |dy| << 16 | (dy + 128) << 8 | (dx + 128).
// cost <= 255 * 256 + 4096 * 246 = 1 072 896 < 2^21; |dx| + |dy| <= 246 < 2^8; |dy| <= 123 < 2^7; dy + 128, dx + 128 < 2^8: 52 bits.
enum { MP_KEY_COST = 31, MP_KEY_MAG = 23, MP_KEY_ADY = 16, MP_KEY_DY = 8 };
__host__ __device__ inline uint64_t pyramid_key(uint32_t cost, int dx, int dy) {
    const uint32_t ax = (uint32_t)(dx < 0 ? -dx : dx), ay = (uint32_t)(dy < 0 ? -dy : dy);
    const uint32_t low = ((ax + ay) << MP_KEY_MAG) | (ay << MP_KEY_ADY) | ((uint32_t)(dy + MP_BIAS) << MP_KEY_DY) | (uint32_t)(dx + MP_BIAS);
    return ((uint64_t)cost << MP_KEY_COST) | low;
}
__host__ __device__ inline void pyramid_unkey(uint64_t key, int smoothness, int* dx, int* dy, int32_t* sad) {
    *dx = (int)(key & 255) - MP_BIAS;
    *dy = (int)((key >> MP_KEY_DY) & 255) - MP_BIAS;
    const uint32_t mag = (uint32_t)(key >> MP_KEY_MAG) & 255;
    *sad = (int32_t)(key >> MP_KEY_COST) - (int32_t)(smoothness * mag);
}

// nullptr, or what is wrong with the three integer parameters
inline const char* pyramid_args_error(int search_range, int smoothness, int match_threshold) {
    if (search_range < MP_MIN_R || search_range > MP_MAX_R || search_range % MP_STEP_R) return "search_range must be a multiple of 4 in 4..120";
    return motion_args_error(0, smoothness, match_threshold);
}

// The workspace's blocks, each on a 256-byte boundary (base == nullptr: the sizes alone): MotionViews' three, then
//   plane[k] [n + 1][h_k][pitch_k] uint8, k = 1, 2: h_k = ceil(h_{k-1} / 2), w_k likewise, pitch_k = w_k rounded up to 4 (the bytes
//            behind w_k are 0); plane[0] is MotionViews' luma
//   vec[k]   [n][Hb_k][Wb_k][2] int8, k = 1, 2: the coarse vector fields (vec[0] is the caller's vec_out)
struct PyramidViews {
    MotionViews m;
    uint8_t* plane[MP_LEVELS];
    int8_t* vec[MP_LEVELS];
    int h[MP_LEVELS], w[MP_LEVELS], pitch[MP_LEVELS], hb[MP_LEVELS], wb[MP_LEVELS];
    size_t bytes;
};
inline PyramidViews pyramid_views(void* base, int n, int h, int w) {
    PyramidViews v;
    v.m = motion_views(base, n, h, w);
    uint8_t* b = (uint8_t*)base;
    size_t o = v.m.bytes;
    auto take = [&](size_t bytes) { uint8_t* p = b ? b + o : nullptr; o += al256(bytes); return p; };
    v.plane[0] = v.m.luma;
    v.vec[0] = nullptr;
    for (int k = 0; k < MP_LEVELS; k++) {
        v.h[k] = k ? (v.h[k - 1] + 1) / 2 : h;
        v.w[k] = k ? (v.w[k - 1] + 1) / 2 : w;
        v.pitch[k] = (v.w[k] + 3) & ~3;
        v.hb[k] = motion_blocks(v.h[k]);
        v.wb[k] = motion_blocks(v.w[k]);
    }
    for (int k = 1; k < MP_LEVELS; k++) v.plane[k] = take(((size_t)n + 1) * v.h[k] * v.pitch[k]);
    for (int k = 1; k < MP_LEVELS; k++) v.vec[k] = (int8_t*)take((size_t)n * v.hb[k] * v.wb[k] * 2);
    v.bytes = o;
    return v;
}

}  // namespace cs
