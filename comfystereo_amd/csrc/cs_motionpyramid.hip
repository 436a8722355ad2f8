// cs_motionpyramid.hip -- the motion-compensated temporal depth filter with a wide-range, coarse-to-fine motion search
// (cs_motion_depth_pyramid; DESIGN.md section 5, "Coarse-to-fine motion search").  Not in the reference.  cs_motiondepth.hip's full
// search costs (2 S + 1)^2 SADs per block and stops at S = 32; here a full search over R / 4 on the quarter-size luma covers
// |dx|, |dy| <= R + 3 (R up to 120), and at most 46 candidates per block refine it on the half- and the full-size luma.
// tools/motion_pyramid_oracle.py states it in numpy.
//
//   L0       = cs_motiondepth.hip's luma;  L(k+1)(y, x) = (a + b + c + d + 2) >> 2 over the 2 x 2 cell of Lk, Lk edge-replicated to
//              even sizes;  blocks 16 x 16 on every level's own plane;  parent(by, bx) = (by >> 1, bx >> 1) one level up
//   level 2    k_motion_search at S = R / 4: the plain matcher
//   level 1, 0 candidates (0, 0) and 2 v + (ex, ey), |ex|, |ey| <= 1, v the vector of the parent and of its up, down, left and right
//              neighbours that exist; admissible if the block, displaced, lies inside the plane; the winner minimises
//              (sad + smoothness (|dx| + |dy|), |dx| + |dy|, |dy|, dy, dx)
//   vec, sad, matched are level 0's; the filter, m and cut are cs_motiondepth.hip's
//
// 6 + n launches on the caller's stream (and one device-to-device copy for n == 1), no wait for the device, no atomics:
//   k_motion_luma<VEC>   cs_motiondepth.hip: plane 0 of the n + 1 frames
//   k_motion_pyramid     grid (quads of plane 2, n + 1): a lane owns four pixels of a row of plane 2, so 2 x 8 of plane 1 and 4 x 16 of
//                      plane 0: sixteen guarded dword loads, one read of L0 for both levels.  An odd plane's last column and row are
//                      replicated in registers; it stores two dwords on each of two rows of plane 1 and one of plane 2, the bytes
//                      behind a plane's width 0.
//   k_motion_search      cs_motiondepth.hip on plane 2, S = R / 4 <= 30: vec into the workspace; its SADs and flags are not wanted and
//                      go where level 0 writes the pass's own afterwards
//   k_motion_refine      twice: level 1 (vec into the workspace), then level 0 (vec, sad, matched).  Grid (ceil(Wb / 4) Hb, n): a
//                      256-thread workgroup owns four horizontally adjacent blocks of frame pair t, a wave each, which share nothing:
//                      every block has its own candidate list.  A wave stages in LDS
//                        s_cur [16][4] dwords        the block's own pixels, bytes outside the plane 0
//                        s_win [6][18][7] dwords     per parent (and for (0, 0)) rows Y0 + 2 vy - 1 .. + 16 of L_{t-1} from column
//                                                    xs = (X0 + 2 vx - 1) & ~3 on: six aligned dwords a row (18 columns and up to 3 of
//                                                    alignment), 0 outside the plane or where the parent does not exist
//                      (lanes 0..4 fetch the five parents' vectors, a shuffle hands them round), then takes the 46 candidates four at
//                      a time: lane = (candidate, row).  A lane reads its row of the block (one 16-byte LDS read) and five dwords
//                      of the candidate's row in its window, four v_alignbyte_b32 by the column's low two bits, four v_sad_u8; rows
//                      behind bh count 0, the reference bytes behind bw are masked.  The pitch of 7 dwords puts a candidate's 16 rows
//                      on 16 banks.  Four xor-shuffles add the rows up, the lane keeps the minimum of pyramid_key
//                      (cs_motionpyramid.h: the order packed into 52 bits; duplicates need no removal, the key is a total order on
//                      (dx, dy)), two more shuffles reduce it over the four candidates in flight, and lane 0 writes the block's result.
//                      Frame 0 without a valid state: zeros and matched.
//   k_temporal_stat, k_temporal_final, k_motion_filter<VEC>   cs_motiondepth.hip's launches, unchanged
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, ROCm 7.2; no kernel spills a vector or scalar register, none
// uses scratch):                       VGPRs  SGPRs  LDS bytes  occupancy (waves / SIMD)
//   k_motion_pyramid                     26     46        0        8
//   k_motion_refine                      40     43    13120        8
#include "cs_common.h"
#include "cs_kernels.h"
#include "cs_motionpyramid.h"

namespace cs {

// four pixels of the next plane: the rounded means of the 2 x 2 cells of eight columns (a0 a1) of one row and (b0 b1) of the next
__device__ __forceinline__ uint32_t down4(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
    const uint32_t M = 0x00ff00ffu, R = 0x00020002u;   // two sums of at most 1022 in the halves of a dword
    const uint32_t s0 = (((a0 & M) + ((a0 >> 8) & M) + (b0 & M) + ((b0 >> 8) & M) + R) >> 2) & M;
    const uint32_t s1 = (((a1 & M) + ((a1 >> 8) & M) + (b1 & M) + ((b1 >> 8) & M) + R) >> 2) & M;
    return (s0 & 0xffu) | ((s0 >> 8) & 0xff00u) | ((s1 & 0xffu) << 16) | ((s1 << 8) & 0xff000000u);
}

// edge replication: where the plane's width `size` is odd and column `size` lies in the dword d of columns col .. col + 3 (col a
// multiple of 4), it takes the byte of column size - 1, which is even and so shares the dword
__device__ __forceinline__ uint32_t replicate_last(uint32_t d, int col, int size) {
    const int i = size - col;
    if (!(size & 1) || i < 0 || i > 3) return d;
    return i == 1 ? (d & 0xffff00ffu) | ((d & 0xffu) << 8) : (d & 0x00ffffffu) | ((d & 0x00ff0000u) << 8);   // (i is odd)
}

__global__ void __launch_bounds__(MD_THREADS) k_motion_pyramid(const uint8_t* __restrict__ l0, int h0, int w0, int p0, uint8_t* __restrict__ l1,
                                                              int h1, int w1, int p1, uint8_t* __restrict__ l2, int h2, int w2, int p2) {
    const size_t qpr = (size_t)p2 / 4, quads = (size_t)h2 * qpr;
    const size_t q = (size_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (q >= quads) return;
    const size_t f = blockIdx.y;
    const int y2 = (int)(q / qpr), x2 = (int)(q - (size_t)y2 * qpr) * 4;   // plane 2: columns x2 .. x2 + 3; plane 1: 2 x2 .. + 7; plane 0: 4 x2 .. + 15
    const uint8_t* src = l0 + f * h0 * p0;
    uint32_t r[4][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int y = min(4 * y2 + j, h0 - 1);   // (only the second row of a cell can lie behind the plane)
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int x = 4 * x2 + 4 * d;
            r[j][d] = replicate_last(x < p0 ? *reinterpret_cast<const uint32_t*>(src + (size_t)y * p0 + x) : 0u, x, w0);
        }
    }
    uint32_t a[2][2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        a[j][0] = down4(r[2 * j][0], r[2 * j][1], r[2 * j + 1][0], r[2 * j + 1][1]);
        a[j][1] = down4(r[2 * j][2], r[2 * j][3], r[2 * j + 1][2], r[2 * j + 1][3]);
    }
    if (2 * y2 + 1 >= h1) { a[1][0] = a[0][0]; a[1][1] = a[0][1]; }   // plane 1's row behind its last: the last, replicated
    uint8_t* d1 = l1 + f * h1 * p1;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int y = 2 * y2 + j;
#pragma unroll
        for (int d = 0; d < 2; d++) {
            const int x = 2 * x2 + 4 * d;
            if (y < h1 && x < p1) *reinterpret_cast<uint32_t*>(d1 + (size_t)y * p1 + x) = a[j][d] & low_bytes(w1 - x);
            a[j][d] = replicate_last(a[j][d], x, w1);
        }
    }
    *reinterpret_cast<uint32_t*>(l2 + f * h2 * p2 + (size_t)y2 * p2 + x2) = down4(a[0][0], a[0][1], a[1][0], a[1][1]) & low_bytes(w2 - x2);
}

// info of a parent or of (0, 0), as the lanes hand it round: bit 16 = it exists, bits 8..15 vy, bits 0..7 vx (int8 each)
enum { MP_EXISTS = 0x10000 };

__global__ void __launch_bounds__(MD_THREADS) k_motion_refine(const uint8_t* __restrict__ plane, int h, int w, int pitch,
                                                             const int8_t* __restrict__ pvec, int php, int pwp, int smoothness, int match_thr,
                                                             const int32_t* __restrict__ valid, int hb, int wb, int groups,
                                                             int8_t* __restrict__ vec, int32_t* __restrict__ sad_out,
                                                             uint8_t* __restrict__ matched) {
    __shared__ __attribute__((aligned(16))) uint32_t s_cur[MP_WAVES][MD_BLOCK * 4];
    __shared__ uint32_t s_win[MP_WAVES][MP_WINDOWS * MP_WIN_ROWS * MP_WIN_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, t = blockIdx.y;
    const int gx = (int)(blockIdx.x % (unsigned)groups), by = (int)(blockIdx.x / (unsigned)groups);
    const int bx = gx * MP_WAVES + wv;
    const bool active = bx < wb;   // (uniform over the wave)
    const size_t out = ((size_t)t * hb + by) * wb + bx;
    if (t == 0 && valid[0] == 0) {   // no predecessor (uniform; no barrier lies in front)
        if (active && lane == 0) {
            vec[2 * out] = 0; vec[2 * out + 1] = 0;
            if (sad_out) { sad_out[out] = 0; matched[out] = 1; }
        }
        return;
    }
    const int X0 = bx * MD_BLOCK, Y0 = by * MD_BLOCK;
    const int bh = min((int)MD_BLOCK, h - Y0), bw = min((int)MD_BLOCK, w - X0);
    const size_t frame = (size_t)h * pitch;
    const uint8_t* ref = plane + (size_t)t * frame;
    const uint8_t* cur = ref + frame;
    int info = 0;
    if (active) {
        if (lane < MP_PARENTS) {   // the parent, up, down, left, right
            const int qy = (by >> 1) + (lane == 1 ? -1 : (lane == 2 ? 1 : 0)), qx = (bx >> 1) + (lane == 3 ? -1 : (lane == 4 ? 1 : 0));
            if (qy >= 0 && qy < php && qx >= 0 && qx < pwp) {
                const int8_t* p = pvec + 2 * (((size_t)t * php + qy) * pwp + qx);
                info = MP_EXISTS | ((int)(uint8_t)p[1] << 8) | (int)(uint8_t)p[0];
            }
        } else if (lane == MP_PARENTS) {
            info = MP_EXISTS;   // (0, 0)
        }
        // the six windows: every lane runs every round, so that the shuffle's source lanes are live
#pragma unroll 1
        for (int i0 = 0; i0 < MP_WINDOWS * MP_WIN_ROWS * MP_WIN_DW; i0 += 64) {
            const int i = i0 + lane;
            const int win = min(i / (MP_WIN_ROWS * MP_WIN_DW), MP_WINDOWS - 1), rem = i - win * (MP_WIN_ROWS * MP_WIN_DW);
            const int r = rem / MP_WIN_DW, d = rem - r * MP_WIN_DW;
            const int pi = __shfl(info, win);
            const int vx2 = 2 * (int)(int8_t)(pi & 255), vy2 = 2 * (int)(int8_t)((pi >> 8) & 255);
            const int y = Y0 + vy2 - 1 + r, x = ((X0 + vx2 - 1) & ~3) + 4 * d;   // (two's complement: & floors)
            if (i < MP_WINDOWS * MP_WIN_ROWS * MP_WIN_DW) {
                uint32_t v = 0u;
                if ((pi & MP_EXISTS) && y >= 0 && y < h && x >= 0 && x < pitch) v = *reinterpret_cast<const uint32_t*>(ref + (size_t)y * pitch + x);
                s_win[wv][(win * MP_WIN_ROWS + r) * MP_WIN_PITCH + d] = v;
            }
        }
        {   // the block's own pixels: lane -> (row, dword)
            const int x = X0 + 4 * (lane & 3), y = Y0 + (lane >> 2);
            uint32_t v = 0u;
            if (y < h && x < pitch) v = *reinterpret_cast<const uint32_t*>(cur + (size_t)y * pitch + x) & low_bytes(w - x);
            s_cur[wv][lane] = v;
        }
    }
    __syncthreads();
    if (!active) return;
    const uint32_t m0 = low_bytes(bw), m1 = low_bytes(bw - 4), m2 = low_bytes(bw - 8), m3 = low_bytes(bw - 12);
    const int r = lane & 15;
    const uint4 c4 = reinterpret_cast<const uint4*>(s_cur[wv])[r];
    unsigned long long best = ~0ull;
#pragma unroll 2
    for (int c0 = 0; c0 < MP_CANDS; c0 += 4) {
        const int ci = c0 + (lane >> 4);
        const int win = min(ci / 9, MP_WINDOWS - 1);
        const int e = ci < 9 * MP_PARENTS ? ci - 9 * win : 4;   // (0, 0) is the centre of its window
        const int ey = e / 3 - 1, ex = e - 3 * (e / 3) - 1;
        const int pi = __shfl(info, win);
        const int vx2 = 2 * (int)(int8_t)(pi & 255), vy2 = 2 * (int)(int8_t)((pi >> 8) & 255);
        const int dx = vx2 + ex, dy = vy2 + ey;
        const bool ok = ci < MP_CANDS && (pi & MP_EXISTS) && X0 + dx >= 0 && X0 + bw + dx <= w && Y0 + dy >= 0 && Y0 + bh + dy <= h;
        const int col = ((X0 + vx2 - 1) & 3) + ex + 1;          // the byte column of the candidate's first pixel in its window: 0..5
        const uint32_t sh = (uint32_t)col & 3u;
        const uint32_t* p = &s_win[wv][(win * MP_WIN_ROWS + ey + 1 + r) * MP_WIN_PITCH + (col >> 2)];
        const uint32_t d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3], d4 = p[4];
        uint32_t sad = 0u;
        sad = __builtin_amdgcn_sad_u8(c4.x, __builtin_amdgcn_alignbyte(d1, d0, sh) & m0, sad);
        sad = __builtin_amdgcn_sad_u8(c4.y, __builtin_amdgcn_alignbyte(d2, d1, sh) & m1, sad);
        sad = __builtin_amdgcn_sad_u8(c4.z, __builtin_amdgcn_alignbyte(d3, d2, sh) & m2, sad);
        sad = __builtin_amdgcn_sad_u8(c4.w, __builtin_amdgcn_alignbyte(d4, d3, sh) & m3, sad);
        if (r >= bh) sad = 0u;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sad += __shfl_xor(sad, o);   // the 16 rows of the candidate
        const unsigned long long key = ok ? pyramid_key(sad + (uint32_t)smoothness * (uint32_t)(abs(dx) + abs(dy)), dx, dy) : ~0ull;
        best = key < best ? key : best;
    }
#pragma unroll
    for (int o = 32; o >= 16; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o);
        best = other < best ? other : best;
    }
    if (lane == 0) {
        int dx, dy;
        int32_t sad;
        pyramid_unkey(best, smoothness, &dx, &dy, &sad);
        vec[2 * out] = (int8_t)dx; vec[2 * out + 1] = (int8_t)dy;
        if (sad_out) {
            sad_out[out] = sad;
            matched[out] = sad <= match_thr * bw * bh ? 1 : 0;
        }
    }
}

size_t pyramid_workspace_bytes(int n, int h, int w) { return pyramid_views(nullptr, n, h, w).bytes; }

hipError_t launch_motion_depth_pyramid(const float* depth, const float* guide, int n, int h, int w, int c, float alpha, float motion_thr,
                                       float cut_thr, int search_range, int smoothness, int match_thr, float* prev_raw, float* prev,
                                       uint8_t* prev_luma, int32_t* valid, float* out, float* m, int32_t* cut, int8_t* vec, int32_t* sad,
                                       uint8_t* matched, void* workspace, hipStream_t stream) {
    const PyramidViews P = pyramid_views(workspace, n, h, w);
    const dim3 block(MD_THREADS);
    launch_motion_luma(guide, n, h, w, P.pitch[0], prev_luma, valid, P.plane[0], stream);
    const size_t quads = (size_t)P.h[2] * (P.pitch[2] / 4);
    hipLaunchKernelGGL(k_motion_pyramid, dim3((unsigned)((quads + MD_THREADS - 1) / MD_THREADS), (unsigned)n + 1), block, 0, stream,
                       (const uint8_t*)P.plane[0], P.h[0], P.w[0], P.pitch[0], P.plane[1], P.h[1], P.w[1], P.pitch[1], P.plane[2], P.h[2], P.w[2],
                       P.pitch[2]);
    // level 2: the plain matcher.  Its SADs and flags are not the pass's: they go where level 0 writes the pass's own, later on this
    // stream (n Hb_2 Wb_2 elements of the n Hb_0 Wb_0)
    launch_motion_search(P.plane[2], n, P.h[2], P.w[2], P.pitch[2], search_range / 4, smoothness, 255, valid, P.vec[2], sad, matched, stream);
    for (int k = 1; k >= 0; k--) {
        const int groups = (P.wb[k] + MP_WAVES - 1) / MP_WAVES;
        hipLaunchKernelGGL(k_motion_refine, dim3((unsigned)groups * (unsigned)P.hb[k], (unsigned)n), block, 0, stream, (const uint8_t*)P.plane[k],
                           P.h[k], P.w[k], P.pitch[k], (const int8_t*)P.vec[k + 1], P.hb[k + 1], P.wb[k + 1], smoothness, match_thr,
                           (const int32_t*)valid, P.hb[k], P.wb[k], groups, k ? P.vec[1] : vec, k ? nullptr : sad, k ? nullptr : matched);
    }
    return launch_motion_filter(depth, n, h, w, c, alpha, motion_thr, cut_thr, prev_raw, prev, prev_luma, valid, out, m, cut, vec, matched, P.m,
                                stream);
}

}  // namespace cs
