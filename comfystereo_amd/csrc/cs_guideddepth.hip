// cs_guideddepth.hip -- image-guided depth upsampling (cs_guided_depth_plan / cs_guided_depth_apply; DESIGN.md section 5, "Guided
// depth upsampling").  Not in the reference, which stretches a smaller depth map bilinearly (every silhouette becomes a ramp):
// joint bilateral upsampling (Kopf, Cohen, Lischinski, Uyttendaele, SIGGRAPH 2007), restated from the paper.  Each full-resolution
// pixel is a weighted mean of the K x K nearest low-resolution depth samples (K = 2R + 1); a sample's weight is a spatial Gaussian
// times a range weight of the L1 distance between the guide's 8-bit colour at the pixel and at the sample's position.
// tools/guided_oracle.py states it in numpy.
//
//   plan (float64, every operation rounded once; depends on h, w, dh, dw, R, sigma_s, sigma_r only):
//     u = ((2x + 1) dw - w) / (2w);  cx[x] = floor(u + 0.5);  wx[x][j] = float32(exp(-(t t) / ((2 sigma_s) sigma_s))), t = (cx[x] + j - R) - u
//     cy, wy likewise;  wr[d] = float32(exp(-(a a) / ((2 sigma_r) sigma_r))), a = d / 255.0, d = 0..765
//     gx[qx] = min(w - 1, ((2 qx + 1) w) / (2 dw)) in integers, gy likewise
//   apply (float32, every operation rounded once: -ffp-contract=off), taps i = 0..K-1 outer, j = 0..K-1 inner:
//     qy = clamp(cy[y] + i - R, 0, dh - 1), qx = clamp(cx[x] + j - R, 0, dw - 1);  ws = wy[y][i] * wx[x][j]
//     d = L1 distance of code(image[y][x]) and code(image[gy[qy]][gx[qx]]);  wg = ws * wr[d];  v = g[qy][qx]
//     num += wg * v; den += wg; ns += ws * v; ds += ws;      out = den > 0 ? num / den : ns / ds
//
// The plan is a device buffer of 4-byte words, made once per geometry by k_guided_plan and read by every apply of that geometry:
//   wr [768] (766 used) | cx [w] | cy [h] | gx [dw] | gy [dh] | wx [w][K] | wy [h][K]
//
//   k_guided_plan             one launch, one thread per entry of cx, cy, gx, gy and wr (a cx / cy thread writes its K weights too)
//   k_guided_apply<R, CM, VEC>  grid (tiles, n).  A 256-thread workgroup owns an output tile of GD_TW x GD_TH = 64 x 16 pixels.  Since
//                      dh <= h and dw <= w, the taps of the tile lie in at most (64 + K - 1) x (16 + K - 1) low-resolution samples,
//                      from clamp(c[first] - R) to clamp(c[last] + R) on either axis (c is monotone).  The workgroup stages the gray
//                      depth of those samples, the packed guide codes gathered at gy / gx and the range table in LDS (rows of
//                      GD_PITCH = 80 words), one barrier; then lane `tid` owns the four pixels x = X0 + 4 (tid & 15) + {0..3} of row
//                      Y0 + (tid >> 4): its own guide pixels from global memory (VEC: three 16-byte loads; else guarded 4-byte
//                      loads, the same pixels), its centres and column weights from the plan (the row's weight per trip of the row
//                      loop, which is not unrolled: that keeps the registers under 96), K * K taps from LDS, one 16-byte store
//                      (else guarded 4-byte stores).  The L1 distance of two packed codes is one v_sad_u8.  VEC needs w % 4 == 0
//                      (every row of a frame then starts on the 16-byte grid, and h * w % 4 == 0 with it) and image and out on
//                      the 16-byte grid.  No atomics, no workspace beyond the plan.
//   LDS reads: ds_read_b32 banks are (a / 4) % 32 and conflicts count within a 32-lane half, here 16 lanes x 4 pixels of two
//   output rows.  At the ratios the pass is for (dw / w <= 1 / 2) a row's 16 lanes read at most 32 consecutive words per tap and
//   pixel slot: no conflict within a row; the half's two rows read the same low-resolution row (identical addresses broadcast)
//   or two rows GD_PITCH = 80 = 16 mod 32 words apart, which at dw / w <= 1 / 4 (16 words per row) fall on disjoint banks.  At
//   the identity ratio lanes l and l + 8 of a row meet on a bank (2-way).  The range table is read at a data-dependent index.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, ROCm 7.2; no kernel spills a vector or scalar register, none
// uses scratch):                       VGPRs  SGPRs  LDS bytes  occupancy (waves / SIMD)
//   k_guided_plan                        32     48        0        8
//   k_guided_apply<1, 1, true>           60     52    17152        8
//   k_guided_apply<1, 1, false>          71     52    17152        7
//   k_guided_apply<1, 3, true>           60     56    17152        8
//   k_guided_apply<1, 3, false>          71     56    17152        7
//   k_guided_apply<1, 0, true>           60     54    17152        8
//   k_guided_apply<1, 0, false>          71     54    17152        7
//   k_guided_apply<2, 1, true>           76     52    17152        6
//   k_guided_apply<2, 1, false>          78     52    17152        6
//   k_guided_apply<2, 3, true>           76     56    17152        6
//   k_guided_apply<2, 3, false>          78     56    17152        6
//   k_guided_apply<2, 0, true>           76     54    17152        6
//   k_guided_apply<2, 0, false>          78     54    17152        6
//   k_guided_apply<3, 1, true>           92     52    17152        5
//   k_guided_apply<3, 1, false>          94     52    17152        5
//   k_guided_apply<3, 3, true>           92     56    17152        5
//   k_guided_apply<3, 3, false>          94     56    17152        5
//   k_guided_apply<3, 0, true>           92     54    17152        5
//   k_guided_apply<3, 0, false>          94     54    17152        5
#include "cs_common.h"
#include "cs_gray4.h"
#include "cs_guidecode.h"
#include "cs_kernels.h"
#include "cs_math.h"

namespace cs {

enum { GD_THREADS = 256, GD_TW = 64, GD_TH = 16, GD_FW = GD_TW + 6, GD_FH = GD_TH + 6, GD_PITCH = 80, GD_WR = 766, GD_WR_WORDS = 768 };

__device__ const unsigned long long d_guided_exp_tab[256] = {CS_EXP_TAB_VALUES};

// The plan's blocks, in words from its start.
struct GuidedViews {
    size_t wr, cx, cy, gx, gy, wx, wy, words;
};
__host__ __device__ __forceinline__ GuidedViews guided_views(int h, int w, int dh, int dw, int radius) {
    const size_t K = 2 * (size_t)radius + 1;
    GuidedViews v;
    v.wr = 0;
    v.cx = GD_WR_WORDS;
    v.cy = v.cx + (size_t)w;
    v.gx = v.cy + (size_t)h;
    v.gy = v.gx + (size_t)dw;
    v.wx = v.gy + (size_t)dh;
    v.wy = v.wx + (size_t)w * K;
    v.words = v.wy + (size_t)h * K;
    return v;
}

size_t guided_plan_bytes(int h, int w, int dh, int dw, int radius) { return al256(guided_views(h, w, dh, dw, radius).words * 4); }

// One entry of cx (or cy) and its K weights: float64, every operation rounded once.
__device__ __forceinline__ void guided_axis(long long x, long long size, long long dsize, int R, double s2, int32_t* __restrict__ c,
                                            float* __restrict__ wt) {
    const long long top = (2 * x + 1) * dsize - size;
    const double u = (double)top / (double)(2 * size);
    const long long ci = (long long)floor(u + 0.5);
    c[x] = (int32_t)ci;
    const int K = 2 * R + 1;
    for (int j = 0; j < K; j++) {
        const double t = (double)(ci + j - R) - u;
        const double e = -(t * t) / s2;
        wt[(size_t)x * K + j] = (float)csm::exp_exact(e, d_guided_exp_tab);
    }
}

__global__ void __launch_bounds__(GD_THREADS) k_guided_plan(int h, int w, int dh, int dw, int R, double sigma_s, double sigma_r,
                                                            uint32_t* __restrict__ plan) {
    const GuidedViews v = guided_views(h, w, dh, dw, R);
    long long i = (long long)blockIdx.x * GD_THREADS + threadIdx.x;
    if (i < w) { guided_axis(i, w, dw, R, (2.0 * sigma_s) * sigma_s, (int32_t*)plan + v.cx, (float*)plan + v.wx); return; }
    i -= w;
    if (i < h) { guided_axis(i, h, dh, R, (2.0 * sigma_s) * sigma_s, (int32_t*)plan + v.cy, (float*)plan + v.wy); return; }
    i -= h;
    if (i < dw) { const long long g = ((2 * i + 1) * w) / (2 * (long long)dw); plan[v.gx + i] = (uint32_t)(g < w - 1 ? g : w - 1); return; }
    i -= dw;
    if (i < dh) { const long long g = ((2 * i + 1) * h) / (2 * (long long)dh); plan[v.gy + i] = (uint32_t)(g < h - 1 ? g : h - 1); return; }
    i -= dh;
    if (i < GD_WR_WORDS) {
        float r = 0.0f;                                       // (the two words behind the table)
        if (i < GD_WR) {
            const double a = (double)i / 255.0;
            r = (float)csm::exp_exact(-(a * a) / ((2.0 * sigma_r) * sigma_r), d_guided_exp_tab);
        }
        ((float*)plan)[v.wr + i] = r;
    }
}

// (guide_code, guide_pack: cs_guidecode.h)
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <int R, int CM, bool VEC>
__global__ void __launch_bounds__(GD_THREADS) k_guided_apply(const float* __restrict__ image, const float* __restrict__ depth, int h, int w,
                                                             int dh, int dw, int c, const uint32_t* __restrict__ plan,
                                                             float* __restrict__ out) {
    constexpr int K = 2 * R + 1;
    __shared__ float s_g[GD_FH * GD_PITCH];
    __shared__ uint32_t s_c[GD_FH * GD_PITCH];
    __shared__ float s_wr[GD_WR_WORDS];
    const GuidedViews pv = guided_views(h, w, dh, dw, R);
    const int32_t* __restrict__ cx = (const int32_t*)plan + pv.cx;
    const int32_t* __restrict__ cy = (const int32_t*)plan + pv.cy;
    const int32_t* __restrict__ gx = (const int32_t*)plan + pv.gx;
    const int32_t* __restrict__ gy = (const int32_t*)plan + pv.gy;
    const float* __restrict__ wx = (const float*)plan + pv.wx;
    const float* __restrict__ wy = (const float*)plan + pv.wy;
    const int tid = threadIdx.x, f = blockIdx.y;
    const unsigned tiles_x = ((unsigned)w + GD_TW - 1) / GD_TW;
    const int X0 = (int)(blockIdx.x % tiles_x) * GD_TW, Y0 = (int)(blockIdx.x / tiles_x) * GD_TH;
    const int tw = min((int)GD_TW, w - X0), th = min((int)GD_TH, h - Y0);   // the tile's live columns and rows
    // the tile's low-resolution footprint: c is monotone, so every tap lies between the first centre - R and the last + R
    const int fx0 = clampi(cx[X0] - R, 0, dw - 1), fy0 = clampi(cy[Y0] - R, 0, dh - 1);
    const int fw = clampi(clampi(cx[X0 + tw - 1] + R, 0, dw - 1) - fx0 + 1, 1, (int)GD_FW);
    const int fh = clampi(clampi(cy[Y0 + th - 1] + R, 0, dh - 1) - fy0 + 1, 1, (int)GD_FH);
    for (int i = tid; i < GD_WR_WORDS; i += GD_THREADS) s_wr[i] = ((const float*)plan)[pv.wr + i];
    const float* img = image + (size_t)f * h * w * 3;
    const float* dep = depth + (size_t)f * dh * dw * (CM == 1 ? 1 : c);
    for (int s = tid; s < fw * fh; s += GD_THREADS) {
        const int ly = s / fw, lx = s - ly * fw;
        const int qy = fy0 + ly, qx = fx0 + lx;
        const float* dp = dep + ((size_t)qy * dw + qx) * (CM == 1 ? 1 : c);
        const float* ip = img + ((size_t)clampi(gy[qy], 0, h - 1) * w + clampi(gx[qx], 0, w - 1)) * 3;   // (clamped: a plan of another geometry reads wrong pixels, not outside the frame)
        s_g[ly * GD_PITCH + lx] = CM == 3 ? gray_of(dp[0], dp[1], dp[2]) : dp[0];
        s_c[ly * GD_PITCH + lx] = guide_pack(ip[0], ip[1], ip[2]);
    }
    __syncthreads();
    const int lx4 = (tid & 15) * 4, lrow = tid >> 4;
    if (lx4 >= tw || lrow >= th) return;                      // (the kernel's only barrier lies behind)
    const int x0 = X0 + lx4, y = Y0 + lrow;
    const size_t base = (size_t)y * w + x0;                    // (VEC: w % 4 == 0, so x0 + 3 < w and base % 4 == 0)
    uint32_t pc[4];
    if (VEC) {
        const float4* q = reinterpret_cast<const float4*>(img + 3 * base);
        const float4 a = q[0], b = q[1], cc = q[2];
        pc[0] = guide_pack(a.x, a.y, a.z); pc[1] = guide_pack(a.w, b.x, b.y);
        pc[2] = guide_pack(b.z, b.w, cc.x); pc[3] = guide_pack(cc.y, cc.z, cc.w);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            pc[k] = 0u;
            if (lx4 + k < tw) pc[k] = guide_pack(img[3 * (base + k)], img[3 * (base + k) + 1], img[3 * (base + k) + 2]);
        }
    }
    // the lane's centres and column weights (a pixel behind the row's end repeats the last one's); the row's weight comes per trip
    float wxv[4][K];
    int cxv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = X0 + min(lx4 + k, tw - 1);
        cxv[k] = cx[x] - R - fx0;
#pragma unroll
        for (int j = 0; j < K; j++) wxv[k][j] = wx[(size_t)x * K + j];
    }
    const int cyv = cy[y] - R;
    const float* __restrict__ wyr = wy + (size_t)y * K;
    const int qx_lo = -fx0, qx_hi = dw - 1 - fx0;              // clamp(cx + j - R, 0, dw - 1) - fx0, in footprint columns
    float num[4], den[4], ns[4], ds[4];
#pragma unroll
    for (int k = 0; k < 4; k++) num[k] = den[k] = ns[k] = ds[k] = 0.0f;
#pragma unroll 1
    for (int i = 0; i < K; i++) {
        const int row = clampi(clampi(cyv + i, 0, dh - 1) - fy0, 0, fh - 1) * GD_PITCH;
        const float wyi = wyr[i];
#pragma unroll
        for (int j = 0; j < K; j++) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int at = row + clampi(clampi(cxv[k] + j, qx_lo, qx_hi), 0, fw - 1);
                const float ws = wyi * wxv[k][j];
                const float v = s_g[at];
                const uint32_t d = __builtin_amdgcn_sad_u8(pc[k], s_c[at], 0u);
                const float wg = ws * s_wr[d];
                num[k] = num[k] + wg * v;
                den[k] = den[k] + wg;
                ns[k] = ns[k] + ws * v;
                ds[k] = ds[k] + ws;
            }
        }
    }
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const bool ranged = den[k] > 0.0f;                    // else every range weight rounded to zero: the spatial mean
        r[k] = (ranged ? num[k] : ns[k]) / (ranged ? den[k] : ds[k]);
    }
    float* o = out + (size_t)f * h * w + base;
    if (VEC) {
        *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (lx4 + k < tw) o[k] = r[k];
    }
}

hipError_t launch_guided_plan(int h, int w, int dh, int dw, int radius, double sigma_s, double sigma_r, void* plan, hipStream_t stream) {
    const size_t entries = (size_t)w + h + dw + dh + GD_WR_WORDS;
    hipLaunchKernelGGL(k_guided_plan, dim3((unsigned)((entries + GD_THREADS - 1) / GD_THREADS)), dim3(GD_THREADS), 0, stream, h, w, dh, dw,
                       radius, sigma_s, sigma_r, (uint32_t*)plan);
    return hipGetLastError();
}

template <int R>
static void guided_apply_r(const float* image, const float* depth, int n, int h, int w, int dh, int dw, int c, const uint32_t* plan,
                           float* out, bool vec, hipStream_t stream) {
    const unsigned tiles = (((unsigned)w + GD_TW - 1) / GD_TW) * (((unsigned)h + GD_TH - 1) / GD_TH);
    const dim3 grid(tiles, (unsigned)n), block(GD_THREADS);
#define CS_GUIDED_APPLY(CM, VEC) \
    hipLaunchKernelGGL((k_guided_apply<R, CM, VEC>), grid, block, 0, stream, image, depth, h, w, dh, dw, c, plan, out)
    if (c == 1) { if (vec) CS_GUIDED_APPLY(1, true); else CS_GUIDED_APPLY(1, false); }
    else if (c == 3) { if (vec) CS_GUIDED_APPLY(3, true); else CS_GUIDED_APPLY(3, false); }
    else { if (vec) CS_GUIDED_APPLY(0, true); else CS_GUIDED_APPLY(0, false); }
#undef CS_GUIDED_APPLY
}

hipError_t launch_guided_apply(const float* image, const float* depth, int n, int h, int w, int dh, int dw, int c, int radius,
                               const void* plan, float* out, hipStream_t stream) {
    const bool vec = vec4_path((size_t)w, {image, out});   // (a lane's pixels lie in one row: every row must start on the grid)
    if (radius == 1) guided_apply_r<1>(image, depth, n, h, w, dh, dw, c, (const uint32_t*)plan, out, vec, stream);
    else if (radius == 2) guided_apply_r<2>(image, depth, n, h, w, dh, dw, c, (const uint32_t*)plan, out, vec, stream);
    else guided_apply_r<3>(image, depth, n, h, w, dh, dw, c, (const uint32_t*)plan, out, vec, stream);
    return hipGetLastError();
}

}  // namespace cs
