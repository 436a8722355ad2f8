// cs_motiondepth.h -- what the host and the device share of the motion-compensated temporal depth filter (cs_motiondepth.hip,
// cs_abi.hip): the block matcher's geometry, the packed key of its order, the parameters' ranges and the workspace's blocks.
// Plain C++ but for the __host__ __device__ marks, so a stand-alone host program can check it (tests/test_motion_depth_host.py).
#pragma once
#include "cs_common.h"
#include "cs_kernels.h"
#include "cs_temporalstat.h"

namespace cs {

enum {
    MD_BLOCK = 16,          // a block's side
    MD_MAX_S = 32,          // the largest search range
    MD_MAX_SMOOTH = 4096,   // the largest smoothness
    MD_THREADS = 256,
    MD_GROUP = 4,           // horizontally adjacent blocks a workgroup of the search serves from one reference window
    MD_ROWS = MD_BLOCK + 2 * MD_MAX_S,                 // 80: the window's rows at the largest search range
    MD_PITCH_DW = (MD_GROUP * MD_BLOCK + 2 * MD_MAX_S + 3) / 4 + 1,   // 33 dwords: 64 + 2 S columns, up to 3 of alignment, the read ahead
};

// The order (cost, |dx| + |dy|, |dy|, dy, dx) as one integer: cost << 27 | (|dx| + |dy|) << 20 | |dy| << 14 | (dy + 32) << 7 | (dx + 32).
// cost <= 255 * 256 + 4096 * 64 = 327 424 < 2^19; |dx| + |dy| <= 64 < 2^7; |dy| <= 32 < 2^6; dy + 32, dx + 32 <= 64 < 2^7: 46 bits.
enum { MD_KEY_COST = 27, MD_KEY_MAG = 20, MD_KEY_ADY = 14, MD_KEY_DY = 7 };
__host__ __device__ inline uint64_t motion_key(uint32_t cost, int dx, int dy) {
    const uint32_t ax = (uint32_t)(dx < 0 ? -dx : dx), ay = (uint32_t)(dy < 0 ? -dy : dy);
    const uint32_t low = ((ax + ay) << MD_KEY_MAG) | (ay << MD_KEY_ADY) | ((uint32_t)(dy + 32) << MD_KEY_DY) | (uint32_t)(dx + 32);
    return ((uint64_t)cost << MD_KEY_COST) | low;
}
__host__ __device__ inline void motion_unkey(uint64_t key, int smoothness, int* dx, int* dy, int32_t* sad) {
    *dx = (int)(key & 127) - 32;
    *dy = (int)((key >> MD_KEY_DY) & 127) - 32;
    const uint32_t mag = (uint32_t)(key >> MD_KEY_MAG) & 127;
    *sad = (int32_t)(key >> MD_KEY_COST) - (int32_t)(smoothness * mag);
}

// nullptr, or what is wrong with the three integer parameters
inline const char* motion_args_error(int search_range, int smoothness, int match_threshold) {
    if (search_range < 0 || search_range > MD_MAX_S) return "search_range must lie in 0..32";
    if (smoothness < 0 || smoothness > MD_MAX_SMOOTH) return "smoothness must lie in 0..4096";
    if (match_threshold < 0 || match_threshold > 255) return "match_threshold must lie in 0..255";
    return nullptr;
}

inline int motion_blocks(int size) { return (size + MD_BLOCK - 1) / MD_BLOCK; }

// the mask of a dword's first `count` bytes, count clamped to 0..4
__host__ __device__ inline uint32_t low_bytes(int count) {
    return count >= 4 ? 0xffffffffu : (count <= 0 ? 0u : (1u << (8 * count)) - 1u);
}

// The workspace's blocks, each on a 256-byte boundary (base == nullptr: the sizes alone):
//   partial  [n][P] float32, the statistic's partial sums (cs_temporalstat.h)
//   luma     [n + 1][h][pitch] uint8, pitch = w rounded up to 4: frame 0 is the state's, frame t + 1 is guide frame t
//   yprev    [h][w] float32: a copy of the state's y for a call of one frame, whose only filter launch reads and writes the state
struct MotionViews {
    float* partial;
    uint8_t* luma;
    float* yprev;
    size_t pitch, bytes;
};
inline MotionViews motion_views(void* base, int n, int h, int w) {
    const size_t hw = (size_t)h * w, pitch = ((size_t)w + 3) & ~(size_t)3;
    uint8_t* b = (uint8_t*)base;
    size_t o = 0;
    auto take = [&](size_t bytes) { uint8_t* p = b ? b + o : nullptr; o += al256(bytes); return p; };
    MotionViews v;
    v.partial = (float*)take((size_t)n * temporal_partials(hw) * 4);
    v.luma = take(((size_t)n + 1) * h * pitch);
    v.yprev = (float*)take(hw * 4);
    v.pitch = pitch;
    v.bytes = o;
    return v;
}

// cs_motiondepth.hip: the pass in its three parts (launch_motion_depth is the three in a row; cs_motionpyramid.hip puts a search of
// its own between the first and the last).  luma: planes [n + 1][h][pitch] of h x w pixels; V: the workspace's views.
void launch_motion_luma(const float* guide, int n, int h, int w, int pitch, const uint8_t* prev_luma, const int32_t* valid, uint8_t* luma,
                        hipStream_t stream);
void launch_motion_search(const uint8_t* luma, int n, int h, int w, int pitch, int search_range, int smoothness, int match_thr,
                          const int32_t* valid, int8_t* vec, int32_t* sad, uint8_t* matched, hipStream_t stream);
hipError_t launch_motion_filter(const float* depth, int n, int h, int w, int c, float alpha, float motion_thr, float cut_thr, float* prev_raw,
                                float* prev, uint8_t* prev_luma, int32_t* valid, float* out, float* m, int32_t* cut, const int8_t* vec,
                                const uint8_t* matched, const MotionViews& V, hipStream_t stream);

}  // namespace cs
