// cs_motiondepth.hip -- motion-compensated temporal depth stabilisation of a video batch (cs_motion_depth; DESIGN.md section 5,
// "Motion-compensated temporal stabilisation").  Not in the reference.  cs_temporal.hip's filter reads y_{t-1} at the pixel itself,
// so whatever moved passes unfiltered; here y_{t-1} is read where the pixel's 16 x 16 block came from, found by a full-search block
// matcher on the 8-bit luma of the clip's colour frames.  tools/motion_oracle.py states it in numpy.
//
//   L      = (77 code(R) + 150 code(G) + 29 code(B) + 128) >> 8 of the guide (code: cs_guidecode.h)
//   v(b)   = the (dx, dy), |dx|, |dy| <= S, block + (dx, dy) inside the frame, that minimises
//            (sad + smoothness (|dx| + |dy|), |dx| + |dy|, |dy|, dy, dx);   sad = sum over the block of |L_t(p) - L_{t-1}(p + (dx, dy))|
//   q      = y_{t-1}(p + v(block(p)));   y_t(p) = g_t(p) if cut_t, sad(v) > match_threshold npix or !(|g_t(p) - q| < motion_threshold),
//            else q + alpha (g_t(p) - q)
// g, m and cut are cs_temporal.hip's (cs_gray4.h, cs_temporalstat.h).  Integer arithmetic in the search, float32 rounded once in
// the filter (-ffp-contract=off).
//
// 3 + n launches on the caller's stream (and one device-to-device copy for n == 1), no wait for the device, no atomics:
//   k_motion_luma<VEC>   grid (quads, n + 1): frame f of the workspace's luma, rows of `pitch` = w rounded up to 4 bytes (the bytes
//                      behind w are 0).  Frame 0 is the state's luma (zeros without a valid state), frame t + 1 is guide frame t.  A
//                      lane owns four pixels of a row and writes one dword; VEC (w % 4 == 0, guide on the 16-byte grid): three
//                      16-byte loads, else guarded 4-byte loads of the same pixels.
//   k_motion_search    grid (ceil(Wb / 4) Hb, n): a 256-thread workgroup owns MD_GROUP = 4 horizontally adjacent blocks of frame pair
//                      t and stages in LDS
//                        s_cur [4][16][4] dwords   the blocks' own pixels, bytes outside the frame 0
//                        s_ref [16 + 2S][33] dwords  rows Y0 - S .. Y0 + 15 + S of L_{t-1}, from column xs = (X0 - S) & ~3 on: the
//                                                  four blocks' windows overlap in all but 16 columns each, so they are staged
//                                                  once (10 560 bytes at S = 32, against 4 x 6 400 for windows of their own);
//                                                  aligned dword loads (pitch and xs are multiples of 4), 0 outside the frame
//                      For each block the 256 lanes take the (2S + 1)^2 candidates c = tid, tid + 256, ... (c = (dy + S)(2S + 1) + dx + S).
//                      A row of a candidate is the block's four dwords (one 16-byte LDS read at a uniform address: a broadcast)
//                      against 16 bytes at byte column 16 b + dx + S + (X0 - S - xs): five aligned dwords, four v_alignbyte_b32 by
//                      the column's low two bits, four v_sad_u8.  Clipped blocks run bh rows and mask the reference bytes behind
//                      bw.  Consecutive lanes have consecutive dx: a wave's reads of one row touch at most 17 consecutive dwords
//                      (four lanes share a dword), and the pitch of 33 puts the next dy's lanes one bank further.  A lane keeps the
//                      minimum of motion_key (cs_motiondepth.h: the order packed into 46 bits), a wave reduces it with six
//                      shuffles, lane 0 of each wave leaves it in s_red[block][wave], and after the kernel's second barrier one
//                      thread per block takes the four in wave order and writes vec, sad and matched.  Frame 0 without a valid
//                      state: zeros and matched.
//   k_temporal_stat, k_temporal_final   cs_temporalstat.h, as in cs_temporal.hip: m, cut, and g into `out` for C != 1
//   k_motion_filter<VEC>  one launch per frame, in order (y_t(p) reads y_{t-1} at other pixels).  A lane owns four pixels of a row,
//                      which lie in one block: its g (16-byte load, else guarded), q through four 4-byte loads at p + v, the
//                      blend, y (16-byte store, else guarded).  The last launch also writes the state: g, y, the frame's luma and
//                      valid = 1.  A call of one frame reads y_{-1} from a copy in the workspace, because that launch writes the
//                      state's y.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, ROCm 7.2; no kernel spills a vector or scalar register, none
// uses scratch):                       VGPRs  SGPRs  LDS bytes  occupancy (waves / SIMD)
//   k_motion_luma<true>                  23     33        0        8
//   k_motion_luma<false>                 11     33        0        8
//   k_motion_search                      58     63    11712        8
//   k_motion_filter<true>                26     42        0        8
//   k_motion_filter<false>               17     40        0        8
// (k_temporal_stat and k_temporal_final compile here to the registers cs_temporal.hip lists for them.)
#include "cs_common.h"
#include "cs_gray4.h"
#include "cs_guidecode.h"
#include "cs_kernels.h"
#include "cs_motiondepth.h"
#include "cs_temporalstat.h"

namespace cs {

__device__ __forceinline__ uint32_t luma_of(float r, float g, float b) {
    return (77u * guide_code(r) + 150u * guide_code(g) + 29u * guide_code(b) + 128u) >> 8;
}

template <bool VEC>
__global__ void __launch_bounds__(MD_THREADS) k_motion_luma(const float* __restrict__ guide, int h, int w, int pitch,
                                                           const uint8_t* __restrict__ prev_luma, const int32_t* __restrict__ valid,
                                                           uint32_t* __restrict__ luma) {
    const size_t qpr = (size_t)pitch / 4, quads = (size_t)h * qpr;
    const size_t q = (size_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (q >= quads) return;
    const int f = blockIdx.y;
    const size_t y = q / qpr;
    const int x4 = (int)(q - y * qpr) * 4;
    const size_t base = y * (size_t)w + x4;
    uint32_t pk = 0u;
    if (f == 0) {   // (uniform over the workgroup)
        if (valid[0] != 0) {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (x4 + k < w) pk |= (uint32_t)prev_luma[base + k] << (8 * k);
        }
    } else {
        const float* img = guide + (size_t)(f - 1) * h * w * 3;
        if (VEC) {
            const float4* p = reinterpret_cast<const float4*>(img + 3 * base);
            const float4 a = p[0], b = p[1], cc = p[2];
            pk = luma_of(a.x, a.y, a.z) | (luma_of(a.w, b.x, b.y) << 8) | (luma_of(b.z, b.w, cc.x) << 16) | (luma_of(cc.y, cc.z, cc.w) << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (x4 + k < w) pk |= luma_of(img[3 * (base + k)], img[3 * (base + k) + 1], img[3 * (base + k) + 2]) << (8 * k);
        }
    }
    luma[(size_t)f * quads + q] = pk;
}

__global__ void __launch_bounds__(MD_THREADS) k_motion_search(const uint8_t* __restrict__ luma, int h, int w, int pitch, int S,
                                                             int smoothness, int match_thr, const int32_t* __restrict__ valid,
                                                             int hb, int wb, int groups, int8_t* __restrict__ vec,
                                                             int32_t* __restrict__ sad_out, uint8_t* __restrict__ matched) {
    __shared__ __attribute__((aligned(16))) uint32_t s_cur[MD_GROUP * MD_BLOCK * 4];
    __shared__ uint32_t s_ref[MD_ROWS * MD_PITCH_DW];
    __shared__ unsigned long long s_red[MD_GROUP][MD_THREADS / 64];
    const int tid = threadIdx.x, t = blockIdx.y;
    const int gx = (int)(blockIdx.x % (unsigned)groups), by = (int)(blockIdx.x / (unsigned)groups);
    const int X0 = gx * MD_GROUP * MD_BLOCK, Y0 = by * MD_BLOCK;
    const int bh = min((int)MD_BLOCK, h - Y0);
    const size_t out0 = ((size_t)t * hb + by) * wb + (size_t)gx * MD_GROUP;
    if (t == 0 && valid[0] == 0) {   // no predecessor (uniform; no barrier lies in front)
        if (tid < MD_GROUP && gx * MD_GROUP + tid < wb) {
            vec[2 * (out0 + tid)] = 0; vec[2 * (out0 + tid) + 1] = 0;
            sad_out[out0 + tid] = 0;
            matched[out0 + tid] = 1;
        }
        return;
    }
    const size_t frame = (size_t)h * pitch;
    const uint8_t* ref = luma + (size_t)t * frame;
    const uint8_t* cur = ref + frame;
    // the window: rows Y0 - S .. Y0 + 15 + S, columns from xs, the multiple of 4 at or below X0 - S (two's complement: & floors)
    const int a = (X0 - S) & 3, xs = X0 - S - a;
    const int rows = MD_BLOCK + 2 * S, ndw = min((int)MD_PITCH_DW, (MD_GROUP * MD_BLOCK + 2 * S + a) / 4 + 1);
    for (int i = tid; i < rows * ndw; i += MD_THREADS) {
        const int r = i / ndw, d = i - r * ndw;
        const int y = Y0 - S + r, x = xs + 4 * d;
        uint32_t v = 0u;
        if (y >= 0 && y < h && x >= 0 && x < pitch) v = *reinterpret_cast<const uint32_t*>(ref + (size_t)y * pitch + x);
        s_ref[r * MD_PITCH_DW + d] = v;
    }
    {   // the four blocks' own pixels: thread -> (block, row, dword)
        const int r = (tid >> 2) & 15, x = X0 + (tid >> 6) * MD_BLOCK + 4 * (tid & 3), y = Y0 + r;
        uint32_t v = 0u;
        if (y < h && x < pitch) v = *reinterpret_cast<const uint32_t*>(cur + (size_t)y * pitch + x) & low_bytes(w - x);
        s_cur[tid] = v;
    }
    __syncthreads();
    const int K = 2 * S + 1, KK = K * K;
#pragma unroll 1
    for (int b = 0; b < MD_GROUP; b++) {
        const int bx = X0 + b * MD_BLOCK, bw = min((int)MD_BLOCK, w - bx);
        if (bw <= 0) break;   // (uniform: the blocks behind the frame's last)
        const uint32_t m0 = low_bytes(bw), m1 = low_bytes(bw - 4), m2 = low_bytes(bw - 8), m3 = low_bytes(bw - 12);
        unsigned long long best = ~0ull;
        for (int c = tid; c < KK; c += MD_THREADS) {
            const int dyi = c / K, dxi = c - dyi * K;
            const int dy = dyi - S, dx = dxi - S;
            if (bx + dx < 0 || bx + bw + dx > w || Y0 + dy < 0 || Y0 + bh + dy > h) continue;
            const int col = b * MD_BLOCK + dxi + a;                // the byte column of the candidate's first pixel in s_ref
            const uint32_t sh = (uint32_t)col & 3u;
            const uint32_t* p = s_ref + dyi * MD_PITCH_DW + (col >> 2);
            const uint4* cu = reinterpret_cast<const uint4*>(s_cur + b * MD_BLOCK * 4);
            uint32_t sad = 0u;
#pragma unroll 4
            for (int r = 0; r < bh; r++) {
                const uint4 c4 = cu[r];
                const uint32_t d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3], d4 = p[4];
                sad = __builtin_amdgcn_sad_u8(c4.x, __builtin_amdgcn_alignbyte(d1, d0, sh) & m0, sad);
                sad = __builtin_amdgcn_sad_u8(c4.y, __builtin_amdgcn_alignbyte(d2, d1, sh) & m1, sad);
                sad = __builtin_amdgcn_sad_u8(c4.z, __builtin_amdgcn_alignbyte(d3, d2, sh) & m2, sad);
                sad = __builtin_amdgcn_sad_u8(c4.w, __builtin_amdgcn_alignbyte(d4, d3, sh) & m3, sad);
                p += MD_PITCH_DW;
            }
            const unsigned long long key = motion_key(sad + (uint32_t)smoothness * (uint32_t)(abs(dx) + abs(dy)), dx, dy);
            best = key < best ? key : best;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o);
            best = other < best ? other : best;
        }
        if ((tid & 63) == 0) s_red[b][tid >> 6] = best;
    }
    __syncthreads();
    if (tid < MD_GROUP) {
        const int bx = X0 + tid * MD_BLOCK, bw = min((int)MD_BLOCK, w - bx);
        if (bw > 0) {
            unsigned long long best = s_red[tid][0];
#pragma unroll
            for (int k = 1; k < MD_THREADS / 64; k++) best = s_red[tid][k] < best ? s_red[tid][k] : best;
            int dx, dy;
            int32_t sad;
            motion_unkey(best, smoothness, &dx, &dy, &sad);
            vec[2 * (out0 + tid)] = (int8_t)dx; vec[2 * (out0 + tid) + 1] = (int8_t)dy;
            sad_out[out0 + tid] = sad;
            matched[out0 + tid] = sad <= match_thr * bw * bh ? 1 : 0;
        }
    }
}

// g and y may be the same array (C != 1: a lane reads its own four g before it writes their y): no __restrict__ on them
template <bool VEC>
__global__ void __launch_bounds__(MD_THREADS) k_motion_filter(const float* g_in, const float* __restrict__ y_prev, float* y_out, int h, int w,
                                                             const int8_t* __restrict__ vec, const uint8_t* __restrict__ matched, int wb,
                                                             const int32_t* __restrict__ cut, float alpha, float motion_thr, int last,
                                                             const uint8_t* __restrict__ luma, int pitch, float* __restrict__ prev_raw,
                                                             float* __restrict__ prev, uint8_t* __restrict__ prev_luma,
                                                             int32_t* __restrict__ valid) {
    const size_t qpr = ((size_t)w + 3) / 4, quads = (size_t)h * qpr;
    const size_t qi = (size_t)blockIdx.x * MD_THREADS + threadIdx.x;
    if (last && qi == 0) valid[0] = 1;   // (nothing in this kernel reads it)
    if (qi >= quads) return;
    const size_t y = qi / qpr;
    const int x4 = (int)(qi - y * qpr) * 4;
    const size_t base = y * (size_t)w + x4;
    // the row's pixels from x4 on as a frame of their own: VEC has w % 4 == 0, so all four are real and base is a multiple of 4
    const size_t left = (size_t)(w - x4);
    const Px4 g = load_gray4<1, VEC>(g_in + base, 0, left, 1);
    const size_t blk = (y / MD_BLOCK) * wb + (size_t)(x4 / MD_BLOCK);
    const int dx = vec[2 * blk], dy = vec[2 * blk + 1];
    const bool keep = cut[0] != 0 || matched[blk] == 0;
    const float* src = y_prev + (size_t)((long long)base + (long long)dy * w + dx);
    Px4 out;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float r = g.v[k];
        if (VEC || x4 + k < w) {
            const float q = src[k];
            const float delta = g.v[k] - q;
            const float blend = q + alpha * delta;
            r = (keep || !(fabsf(delta) < motion_thr)) ? g.v[k] : blend;
        }
        out.v[k] = r;
    }
    store4<VEC>(y_out + base, 0, left, out);
    if (last) {
        store4<VEC>(prev_raw + base, 0, left, g);
        store4<VEC>(prev + base, 0, left, out);
        const uint32_t pk = *reinterpret_cast<const uint32_t*>(luma + y * (size_t)pitch + x4);
        if (VEC) {
            *reinterpret_cast<uint32_t*>(prev_luma + base) = pk;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (x4 + k < w) prev_luma[base + k] = (uint8_t)(pk >> (8 * k));
        }
    }
}

size_t motion_workspace_bytes(int n, int h, int w) { return motion_views(nullptr, n, h, w).bytes; }

// The pass in its three parts, which cs_motionpyramid.hip launches as well, with a search of its own between the first and the last.

// the luma of the whole batch: luma [n + 1][h][pitch], frame 0 the state's
void launch_motion_luma(const float* guide, int n, int h, int w, int pitch, const uint8_t* prev_luma, const int32_t* valid, uint8_t* luma,
                        hipStream_t stream) {
    const size_t quads = (size_t)h * (pitch / 4);
    const dim3 block(MD_THREADS), lgrid((unsigned)((quads + MD_THREADS - 1) / MD_THREADS), (unsigned)n + 1);
    if (vec4_path((size_t)w, {guide}))
        hipLaunchKernelGGL(k_motion_luma<true>, lgrid, block, 0, stream, guide, h, w, pitch, prev_luma, valid, (uint32_t*)luma);
    else
        hipLaunchKernelGGL(k_motion_luma<false>, lgrid, block, 0, stream, guide, h, w, pitch, prev_luma, valid, (uint32_t*)luma);
}

// every frame pair's vectors by full search on planes [n + 1][h][pitch] of h x w pixels: they depend on the guide alone
void launch_motion_search(const uint8_t* luma, int n, int h, int w, int pitch, int search_range, int smoothness, int match_thr,
                          const int32_t* valid, int8_t* vec, int32_t* sad, uint8_t* matched, hipStream_t stream) {
    const int hb = motion_blocks(h), wb = motion_blocks(w), groups = (wb + MD_GROUP - 1) / MD_GROUP;
    hipLaunchKernelGGL(k_motion_search, dim3((unsigned)groups * (unsigned)hb, (unsigned)n), dim3(MD_THREADS), 0, stream, luma, h, w, pitch,
                       search_range, smoothness, match_thr, valid, hb, wb, groups, vec, sad, matched);
}

// m, cut and the filter along the vectors; V: the workspace's partial, luma and yprev
hipError_t launch_motion_filter(const float* depth, int n, int h, int w, int c, float alpha, float motion_thr, float cut_thr, float* prev_raw,
                                float* prev, uint8_t* prev_luma, int32_t* valid, float* out, float* m, int32_t* cut, const int8_t* vec,
                                const uint8_t* matched, const MotionViews& V, hipStream_t stream) {
    const size_t hw = (size_t)h * w, quads = (size_t)h * (V.pitch / 4);
    const int pitch = (int)V.pitch, hb = motion_blocks(h), wb = motion_blocks(w);
    const dim3 block(MD_THREADS), qgrid((unsigned)((quads + MD_THREADS - 1) / MD_THREADS));
    // m and cut, and g into `out` for C != 1: the plain filter's statistic, on the plain filter's choice of its path
    launch_temporal_stat(depth, n, hw, c, cut_thr, prev_raw, valid, out, m, cut, V.partial, vec4_path(hw, {depth, out, prev_raw, prev}), stream);
    const float* y_first = prev;
    if (n == 1) {   // the only filter launch writes the state's y: it reads a copy
        hipError_t e = hipMemcpyAsync(V.yprev, prev, hw * 4, hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return e;
        y_first = V.yprev;
    }
    const bool fvec = vec4_path((size_t)w, {depth, out, prev_raw, prev}) && ((uintptr_t)prev_luma & 3) == 0;
    const size_t blocks = (size_t)hb * wb;
    for (int t = 0; t < n; t++) {
        const float* g_in = c == 1 ? depth + (size_t)t * hw : out + (size_t)t * hw;
        const float* y_prev = t > 0 ? out + (size_t)(t - 1) * hw : y_first;
        const uint8_t* lum = V.luma + (size_t)(t + 1) * h * V.pitch;
        const int last = t == n - 1;
#define CS_MOTION_FILTER(VEC) \
        hipLaunchKernelGGL(k_motion_filter<VEC>, qgrid, block, 0, stream, g_in, y_prev, out + (size_t)t * hw, h, w, vec + 2 * t * blocks, \
                           matched + t * blocks, wb, (const int32_t*)cut + t, alpha, motion_thr, last, lum, pitch, prev_raw, prev,        \
                           prev_luma, valid)
        if (fvec) CS_MOTION_FILTER(true); else CS_MOTION_FILTER(false);
#undef CS_MOTION_FILTER
    }
    return hipGetLastError();
}

hipError_t launch_motion_depth(const float* depth, const float* guide, int n, int h, int w, int c, float alpha, float motion_thr,
                               float cut_thr, int search_range, int smoothness, int match_thr, float* prev_raw, float* prev,
                               uint8_t* prev_luma, int32_t* valid, float* out, float* m, int32_t* cut, int8_t* vec, int32_t* sad,
                               uint8_t* matched, void* workspace, hipStream_t stream) {
    const MotionViews V = motion_views(workspace, n, h, w);
    launch_motion_luma(guide, n, h, w, (int)V.pitch, prev_luma, valid, V.luma, stream);
    launch_motion_search(V.luma, n, h, w, (int)V.pitch, search_range, smoothness, match_thr, valid, vec, sad, matched, stream);
    return launch_motion_filter(depth, n, h, w, c, alpha, motion_thr, cut_thr, prev_raw, prev, prev_luma, valid, out, m, cut, vec, matched, V,
                                stream);
}

}  // namespace cs
